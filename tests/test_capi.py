"""CPU-side checks of the C-ABI boundary: the library loads, exports every symbol that
include/vampire_hip.h declares, rejects bad descriptors without touching a GPU, and the
Python host refuses CPU tensors (there is no fallback)."""
import ctypes as C
import re

import pytest
import torch

from vampire_amd import _capi, _header
from vampire_amd.build import build_library


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def header_symbols():
    return sorted(_header.read().prototypes)


def test_exports_every_declared_symbol(lib):
    names = header_symbols()
    assert len(names) >= 15
    raw = C.CDLL(_capi.lib_path())
    for n in names:
        assert hasattr(raw, n), f"{n} declared in vampire_hip.h but not exported"
    assert set(names) == set(_capi.SIGNATURES), "ctypes binding out of sync with the header"
    assert lib.vamp_abi_version() == _capi.ABI_VERSION


def test_struct_layout_matches_header(lib):
    # 9+... ints and floats, no padding surprises: sizes are part of the ABI
    assert C.sizeof(_capi.VampLiftDesc) == 18 * 4
    assert C.sizeof(_capi.VampRenderDesc) == 29 * 4
    assert C.sizeof(_capi.VampSampleDesc) == 22 * 4
    assert C.sizeof(_capi.VampConvDesc) == 6 * 4
    assert C.sizeof(_capi.VampBevBackwardPlan) == 40 * 4
    assert C.sizeof(_capi.VampCameraForwardPlan) == 16 * 4
    assert C.sizeof(_capi.VampCameraBackwardPlan) == 28 * 4
    assert C.sizeof(_capi.VampRenderWorkspaceLayout) == (2 * 19 + 2) * 8
    assert C.sizeof(_capi.VampLiftForwardPlan) == 22 * 4
    assert C.sizeof(_capi.VampLiftBackwardPlan) == 32 * 4
    assert C.sizeof(_capi.VampLiftWorkspaceLayout) == (2 * 13 + 1) * 8


def test_bad_descriptor_is_rejected_without_gpu(lib):
    d = _capi.VampLiftDesc()          # all zeros
    rc = lib.vamp_lift_indices(C.byref(d), None, None, None, None, None, None, None, None, None)
    assert rc == -1
    assert b"requirement failed" in lib.vamp_last_error()
    rd = _capi.VampRenderDesc()
    assert lib.vamp_frustum_geometry(C.byref(rd), None, None, None, None, None, None) == -1
    assert lib.vamp_lift_workspace_bytes(None) == 0


def test_missing_library_is_loud(monkeypatch):
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setenv("VAMPIRE_HIP_LIB", "/nonexistent/libvampire_hip.so")
    with pytest.raises(_capi.VampireHipError):
        _capi.load()
    monkeypatch.delenv("VAMPIRE_HIP_LIB")
    monkeypatch.setattr(_capi, "_lib", None)
    _capi.load()


def test_cpu_tensors_are_refused():
    """The product path must fail loudly rather than fall back to a CPU implementation."""
    from vampire_amd.config import CFG_TINY
    from vampire_amd.ops import _chk
    with pytest.raises(_capi.VampireHipError):
        _chk(torch.zeros(2, 2), (2, 2), "x")
    from vampire_amd import ops
    from vampire_amd.ops import HotPath
    with pytest.raises(_capi.VampireHipError):
        ops.upsample_trilinear(torch.zeros(1, 1, 2, 2, 2), (4, 4, 4))
    with pytest.raises(_capi.VampireHipError):
        ops.conv3d_3x3x3(torch.zeros(1, 16, 2, 2, 2), torch.zeros(16, 16, 3, 3, 3))


def test_new_entry_points_reject_bad_arguments_without_gpu(lib):
    """The widening rows' entry points validate before touching the device."""
    cd = _capi.VampConvDesc()
    cd.B, cd.cin, cd.cout, cd.Z, cd.Y, cd.X = 1, 8, 16, 4, 4, 4           # 8 input channels: unsupported
    assert lib.vamp_conv3d_forward(C.byref(cd), None, None, None, None) == -1
    assert b"cin, cout must be 16 or 32" in lib.vamp_last_error()
    assert lib.vamp_conv3d_workspace_bytes(C.byref(cd)) == 0
    assert lib.vamp_conv3d_supported(C.byref(cd)) == 0
    cd.cin, cd.X = 32, 256                                                  # cfg-A's conv6 row: supported
    assert lib.vamp_conv3d_supported(C.byref(cd)) == 1
    cd.X = 400                                                              # cfg-D: row too long
    assert lib.vamp_conv3d_supported(C.byref(cd)) == 0
    assert lib.vamp_upsample_trilinear_forward(0, 1, 1, 1, 2, 2, 2, None, None, None) == -1
    assert lib.vamp_depth_softmax_forward(1, 0, 4, None, 0, None, None) == -1
    assert lib.vamp_density_gate_forward(1, 4, 8, 7, None, None, None, None) == -1


RENDER_ENTRIES = ["vamp_render_camera_forward_ex", "vamp_render_camera_backward_acc", "vamp_render_bev_forward_ex",
                  "vamp_render_forward_merged", "vamp_render_camera_terminate", "vamp_render_camera_prepare_ex"]


def _null_args(fn, d):
    """A descriptor and nothing else: NULL for every pointer, 0 for every count and flag word."""
    simple = (C.c_int, C.c_size_t, C.c_float, C.c_long)
    return [C.byref(d)] + [0 if t in simple else None for t in fn.argtypes[1:]]


@pytest.mark.parametrize("field,value,message", [("K", 0, b"1 <= K <= 28"), ("K", 29, b"1 <= K <= 28"),
                                                 ("C", 65, b"0 <= C <= 64"), ("D", 1, b"D > 1")])
def test_render_descriptor_limits_are_rejected_without_gpu(lib, field, value, message):
    """The render entry points refuse a class count outside 1 .. 28, more than 64 mid channels or a single depth plane
    with a negative code and the descriptor check's message, before any device work (every pointer is NULL: a call
    that went on would fail differently); the same calls on the valid descriptor stop at their pointer checks."""
    from vampire_amd.config import CFG_TINY
    from vampire_amd.ops import render_desc
    ok = render_desc(CFG_TINY, 2, 6, _capi.VAMP_F32)
    heights = (C.c_float * 3)(-0.0, 0.8, 1.6)
    for name in RENDER_ENTRIES:
        fn = getattr(lib, name)
        assert fn(*_null_args(fn, ok)) < 0, name
        err = lib.vamp_last_error()
        assert (b"null pointer" in err or b"need geom" in err or b"workspace 0 <" in err), (name, err)
    bad = render_desc(CFG_TINY, 2, 6, _capi.VAMP_F32)
    setattr(bad, field, value)
    for name in RENDER_ENTRIES:
        fn = getattr(lib, name)
        assert fn(*_null_args(fn, bad)) < 0, name
        assert message in lib.vamp_last_error(), (name, lib.vamp_last_error())
    assert lib.vamp_render_forward_merged_supported(C.byref(bad), heights) == 0
    assert lib.vamp_render_workspace_bytes(C.byref(ok)) > 0


# ------------------------------------------------------------------ the binding's conversions (CPU tensors only)
def _as_address(converted):
    """What ctypes puts on the stack for a TensorPtr argument: None is NULL, otherwise the 64-bit value."""
    return 0 if converted is None else (C.cast(converted, C.c_void_p).value or 0)


def test_tensor_pointer_passes_a_full_64_bit_address():
    """A tensor goes in as its data_ptr(), as a c_void_p: a bare int from from_param would travel as a 32-bit C int."""
    t = torch.arange(5, dtype=torch.int64)
    assert t.data_ptr() >= 2 ** 32, "the host heap lies above 4 GiB on every 64-bit Linux this runs on"
    got = _capi.TensorPtr.from_param(t)
    assert isinstance(got, C.c_void_p) and got.value == t.data_ptr()
    high = _capi.TensorPtr.from_param(0xfedc_ba98_7654_3210)
    assert isinstance(high, C.c_void_p) and high.value == 0xfedc_ba98_7654_3210
    # through a real foreign call: memcpy with TensorPtr parameters copies between the two tensors
    libc = C.CDLL(None)
    memcpy = libc["memcpy"]
    memcpy.restype, memcpy.argtypes = C.c_void_p, [_capi.TensorPtr, _capi.TensorPtr, C.c_size_t]
    dst = torch.zeros(5, dtype=torch.int64)
    assert memcpy(dst, t, 40) == dst.data_ptr()
    assert torch.equal(dst, t)


def test_tensor_pointer_accepts_none_parameters_and_pointers():
    assert _as_address(_capi.TensorPtr.from_param(None)) == 0
    p = torch.nn.Parameter(torch.ones(3))
    assert _capi.TensorPtr.from_param(p).value == p.data_ptr()
    assert _as_address(_capi.TensorPtr.from_param(C.c_void_p(1 << 40))) == 1 << 40
    arr = (C.c_int32 * 2)()
    assert _as_address(_capi.TensorPtr.from_param(arr)) == C.addressof(arr)


def test_tensor_pointer_refuses_other_objects(lib):
    d = _capi.VampLiftDesc()
    for bad in ("a string", 1.5, [1, 2], object()):
        with pytest.raises(C.ArgumentError):
            lib.vamp_lift_indices(d, bad, None, None, None, None, None, None, None, None)


def test_checked_call_raises_where_the_raw_call_returns_the_code(lib):
    d = _capi.VampLiftDesc()          # all zeros, passed without byref
    args = (d, None, None, None, None, None, None, None, None, None)
    with pytest.raises(_capi.VampireHipError) as e:
        _capi.checked().vamp_lift_indices(*args)
    assert str(e.value).startswith("vamp_lift_indices failed with code -1:")
    assert "requirement failed" in str(e.value)
    assert lib.vamp_lift_indices(*args) == -1
    assert lib.vamp_lift_indices is not _capi.checked().vamp_lift_indices


def test_every_signature_is_a_status_or_a_value(lib):
    vamp = _capi.checked()
    for name, (ret, args) in _capi.SIGNATURES.items():
        assert ret.is_status in (True, False), name
        assert ret.ctype is C.c_int or not ret.is_status, f"{name}: a status is a C int"
        fn = getattr(vamp, name)
        assert (fn.errcheck is not None) == ret.is_status if hasattr(fn, "errcheck") else not ret.is_status, name
        assert fn.restype is getattr(lib, name).restype and fn.argtypes == getattr(lib, name).argtypes, name
    values = {n for n, (ret, _) in _capi.SIGNATURES.items() if not ret.is_status}
    assert {"vamp_abi_version", "vamp_profile_slots", "vamp_last_error"} <= values
    assert {n for n in _capi.SIGNATURES if n.endswith(("_supported", "_bytes", "_offset"))} <= values
    # the value returns come back as they are, 0 included, without raising
    assert vamp.vamp_abi_version() == _capi.ABI_VERSION
    cd = _capi.VampConvDesc(1, 8, 16, 4, 4, 4)
    assert vamp.vamp_conv3d_supported(cd) == 0 and vamp.vamp_conv3d_bf16_supported(cd) == 0
    assert vamp.vamp_upsample_trilinear_supported(0, 0, 0, 0, 0, 0) == 0
    assert vamp.vamp_gate_conv1x1_supported(0, 0, 0) == 0
    assert vamp.vamp_render_forward_merged_supported(_capi.VampRenderDesc(), None) == 0


def test_checked_set_follows_a_reload(monkeypatch):
    first = _capi.checked()
    assert _capi.checked() is first
    monkeypatch.setattr(_capi, "_lib", None)
    again = _capi.checked()
    assert again is not first and again.vamp_abi_version() == _capi.ABI_VERSION


def test_checked_calls_go_through_a_stand_in_library(lib):
    """HotPath.lib can be replaced by an object that wraps the library (the sweeps' call recorders): the checked set
    made from it calls through it, and still raises."""
    seen = []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            return lambda *a: (seen.append(name), fn(*a))[1]

    vamp = _capi.checked(Recorder())
    assert vamp.vamp_abi_version() == _capi.ABI_VERSION
    with pytest.raises(_capi.VampireHipError, match="vamp_frustum_geometry failed with code -1"):
        vamp.vamp_frustum_geometry(_capi.VampRenderDesc(), None, None, None, None, None, None)
    assert seen == ["vamp_abi_version", "vamp_frustum_geometry"]
    assert _capi.checked(lib) is _capi.checked()


def test_descriptor_parameters_are_typed_pointers():
    """Every `const VampXDesc*` (or VampDetTask*) parameter of the header is a POINTER(VampXDesc) in the table, so that
    a bare structure instance is passed by reference -- a void* parameter would refuse it."""
    seen = 0
    for name, (_, params) in _header.read().prototypes.items():
        for i, (ctype, _) in enumerate(params):
            m = re.fullmatch(r"const (Vamp\w+)\*", ctype)
            if m:
                seen += 1
                want = C.POINTER(getattr(_capi, m.group(1)))
                assert _capi.SIGNATURES[name][1][i] is want, f"{name}: parameter {i} should be POINTER({m.group(1)})"
    assert seen >= 60
    pd = _capi.VampPoolDesc(1, 4, 16, 0, 4, 1, _capi.VAMP_F32)         # an empty grid, passed without byref
    assert _capi.checked().vamp_voxel_pooling_workspace_bytes(pd) == 0
    assert _capi.load().vamp_voxel_pooling_workspace_bytes(C.byref(pd)) == 0
