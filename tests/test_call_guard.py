"""CPU checks of tests/call_guard.py: its table against the prototypes of include/vampire_hip.h, and the guard itself on
CPU tensors in front of a stand-in library (no GPU: nothing is launched)."""
import inspect
import re

import pytest
import torch

import call_guard as CG
from call_guard import CallGuard, ContractViolation
from vampire_amd import _capi, ops
from vampire_amd.build import build_library
from vampire_amd.config import CFG_TINY


# ---------------------------------------------------------------------------------------------------- table against header
def test_every_table_entry_is_a_header_parameter():
    protos = CG.header_prototypes()
    assert set(protos) == set(_capi.SIGNATURES), "the prototype parser and the binding disagree on the header's symbols"
    for fn, plist in protos.items():
        assert len(plist) == len(_capi.SIGNATURES[fn][1]), f"{fn}: parsed {len(plist)} parameters"
    assert len(CG.TABLE) >= 250
    for fn, pname in CG.TABLE:
        assert fn in protos, f"{fn} is not declared in the header"
        assert pname in [p for _, p in protos[fn]], f"{fn} has no parameter {pname}"
    for fn, (family, ws) in CG.FUNCTIONS.items():
        assert fn in protos, f"{fn} is not declared in the header"
        if ws is not None:
            for pname in CG.WORKSPACE[ws]:
                # (a family's workspace list may name one a member lacks, never one no member has)
                assert any((f, pname) in CG.TABLE for f, (_, w) in CG.FUNCTIONS.items() if w == ws), (ws, pname)


def test_every_tensor_parameter_of_the_covered_functions_is_in_the_table():
    """A pointer parameter is in the table or in the commented exclusions: a renamed or added one fails here."""
    protos = CG.header_prototypes()
    for fn in CG.FUNCTIONS:
        for ctype, pname in protos[fn]:
            if not ctype.endswith("*"):
                assert (fn, pname) not in CG.TABLE, f"{fn}({pname}) is a {ctype}, not a pointer"
                continue
            assert ((fn, pname) in CG.TABLE) != (pname in CG.EXCLUDED), \
                f"{fn}: pointer parameter `{ctype} {pname}` is neither in the table nor excluded (or both)"
            if pname in CG.EXCLUDED:
                assert ("Desc" in ctype or ctype in ("void*", "const float*", "int32_t*")), (fn, ctype, pname)
    # a workspace is always followed by its size
    for (fn, pname), spec in CG.TABLE.items():
        if spec[0] == "workspace":
            names = [p for _, p in protos[fn]]
            assert names[names.index(pname) + 1] == spec[1], (fn, pname)


def test_the_table_covers_every_entry_point_the_operators_call_with_tensors():
    """Every `vamp.vamp_*` call in ops.py is a covered function or a host-only query (sizes, layouts, plans, support)."""
    called = set(re.findall(r"\.vamp\.(vamp_[a-z_0-9]+)\(", inspect.getsource(ops)))
    called |= set(re.findall(r"ask\.(vamp_[a-z_0-9]+)\(", inspect.getsource(ops)))
    assert len(called) >= 30
    host_only = {n for n in called if n.endswith(("_bytes", "_supported", "_layout", "_offset", "_plan"))}
    assert called - host_only <= set(CG.FUNCTIONS), sorted(called - host_only - set(CG.FUNCTIONS))


# ---------------------------------------------------------------------------------------------------- the guard on CPU tensors
class _StandIn:
    """The library's host-only size queries; every other entry point is recorded and returns VAMP_OK unrun."""

    def __init__(self):
        build_library(verbose=False)
        self._real, self.called = _capi.checked(), []

    def __getattr__(self, name):
        if name.endswith(("_bytes", "_supported")):
            return getattr(self._real, name)
        return lambda *a: (self.called.append(name), 0)[1]


@pytest.fixture(scope="module")
def stand_in():
    return _StandIn()


def _lift_call(d, B=2, N=6, C_=4, ws_bytes=None, stand=None):
    c = CFG_TINY
    ws_bytes = stand.vamp_lift_workspace_bytes(d) if ws_bytes is None else ws_bytes
    return dict(d=d, mats=torch.zeros(B, N, 3, 4, 4), xs=torch.zeros(c.vX), ys=torch.zeros(c.vY), zs=torch.zeros(c.vZ),
                depth=torch.zeros(B, N, c.D, c.fH, c.fW), feat=torch.zeros(B, N, C_, c.fH, c.fW),
                out=torch.zeros(B, C_, c.vZ, c.vY, c.vX), hits=torch.zeros(B, c.vZ, c.vY, c.vX, 1, dtype=torch.int64),
                workspace=torch.zeros(ws_bytes, dtype=torch.uint8), workspace_bytes=ws_bytes, flags=0, stream=None)


def _violation(guard, fn, kw, **change):
    kw = dict(kw, **change)
    before = len(guard.log)
    with pytest.raises(ContractViolation) as e:
        getattr(guard, fn)(*kw.values())
    assert len(guard.log) == before
    return e.value


def test_guard_flags_strided_short_host_and_wrong_dtype_tensors(stand_in):
    """(The device check is set to "expect cpu" for this test only: the tensors are CPU tensors.)"""
    guard = CallGuard(stand_in, "cpu", sizes=stand_in)
    d = ops.lift_desc(CFG_TINY, 2, 6, 4, _capi.VAMP_F32)
    kw = _lift_call(d, stand=stand_in)
    fn = "vamp_lift_forward_ex"
    n0 = len(stand_in.called)
    assert guard.vamp_lift_forward_ex(*kw.values()) == 0
    assert [n for n, _ in guard.log] == [fn] and stand_in.called[n0:] == [fn]
    big = torch.zeros(2, 12, CFG_TINY.D, CFG_TINY.fH, CFG_TINY.fW)
    v = _violation(guard, fn, kw, depth=big[:, :6])                                         # a camera subset at B > 1
    assert (v.function, v.parameter) == (fn, "depth") and v.reason.startswith("layout")
    v = _violation(guard, fn, kw, depth=kw["depth"].transpose(3, 4).contiguous().transpose(3, 4))
    assert v.parameter == "depth" and v.reason.startswith("layout")
    v = _violation(guard, fn, kw, depth=kw["depth"][:, :, :1].expand_as(kw["depth"]))
    assert v.parameter == "depth" and v.reason.startswith("layout")
    v = _violation(guard, fn, kw, depth=torch.zeros(2, 6, CFG_TINY.D - 1, CFG_TINY.fH, CFG_TINY.fW))      # short
    assert v.parameter == "depth" and v.reason.startswith("size")
    v = _violation(guard, fn, kw, depth=torch.zeros(2, 6, CFG_TINY.D + 1, CFG_TINY.fH, CFG_TINY.fW))
    assert v.parameter == "depth" and v.reason.startswith("size")
    v = _violation(guard, fn, kw, feat=kw["feat"].bfloat16())                               # bf16 bytes, fp32 code
    assert v.parameter == "feat" and v.reason.startswith("dtype")
    v = _violation(guard, fn, kw, depth=kw["depth"].long())
    assert v.parameter == "depth" and v.reason.startswith("dtype")
    v = _violation(guard, fn, kw, out=kw["out"].double())                                   # a float* parameter
    assert v.parameter == "out" and v.reason.startswith("dtype")
    v = _violation(guard, fn, kw, mats=torch.zeros(2 * 6 * 48 + 1)[1:].view(2, 6, 3, 4, 4))  # one element into a buffer
    assert v.parameter == "mats" and v.reason.startswith("alignment")
    v = _violation(guard, fn, kw, workspace=kw["workspace"][:-1])
    assert v.parameter == "workspace" and v.reason.startswith("size")
    v = _violation(guard, fn, kw, workspace=kw["workspace"][:-256], workspace_bytes=kw["workspace_bytes"] - 256)
    assert v.parameter == "workspace" and v.reason.startswith("size")
    # a host tensor where the call runs on a device
    on_gpu = CallGuard(stand_in, "cuda:0", sizes=stand_in)
    v = _violation(on_gpu, fn, kw)
    assert v.parameter == "mats" and v.reason.startswith("device")
    # bf16 descriptor: the same bf16 tensors pass, fp32 ones do not
    db = ops.lift_desc(CFG_TINY, 2, 6, 4, _capi.VAMP_BF16)
    kb = dict(kw, d=db, depth=kw["depth"].bfloat16(), feat=kw["feat"].bfloat16())
    assert guard.vamp_lift_forward_ex(*kb.values()) == 0
    assert _violation(guard, fn, kb, depth=kw["depth"]).parameter == "depth"
    assert stand_in.called[n0:] == [fn, fn]               # nothing the guard refused reached the library


def test_guard_takes_channel_last_features_under_the_flag_only(stand_in):
    guard = CallGuard(stand_in, "cpu", sizes=stand_in)
    d = ops.lift_desc(CFG_TINY, 2, 6, 4, _capi.VAMP_F32)
    kw = _lift_call(d, stand=stand_in)
    fn = "vamp_lift_forward_ex"
    cl = kw["feat"].permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)
    assert _violation(guard, fn, kw, feat=cl).reason.startswith("layout")
    flag = _capi.VAMP_LIFTFWD_FEAT_CHANNEL_LAST
    assert guard.vamp_lift_forward_ex(*dict(kw, feat=cl, flags=flag).values()) == 0
    assert _violation(guard, fn, kw, flags=flag).reason.startswith("layout")                  # channel-first under the flag
    n = cl.numel()
    off = torch.zeros(n + 1)[1:].view(2, 6, CFG_TINY.fH, CFG_TINY.fW, 4).permute(0, 1, 4, 2, 3)
    assert _violation(guard, fn, kw, feat=off, flags=flag).reason.startswith("alignment")


def test_guard_reads_the_dtype_code_argument_and_the_scalar_dimensions(stand_in):
    guard = CallGuard(stand_in, "cpu", sizes=stand_in)
    lg, out = torch.zeros(12, 21, 8 * 22, dtype=torch.bfloat16), torch.zeros(12, 21, 8 * 22)
    assert guard.vamp_depth_softmax_forward(12, 21, 8 * 22, lg, _capi.VAMP_BF16, out, None) == 0
    v = _violation(guard, "vamp_depth_softmax_forward",
                   dict(images=12, D=21, HW=8 * 22, logits=lg, in_dtype=_capi.VAMP_F32, depth=out, stream=None))
    assert v.parameter == "logits" and v.reason.startswith("dtype")
    v = _violation(guard, "vamp_depth_softmax_forward",
                   dict(images=12, D=22, HW=8 * 22, logits=lg, in_dtype=_capi.VAMP_BF16, depth=out, stream=None))
    assert v.parameter == "logits" and v.reason.startswith("size")
    # gate conv: weight [Cout, C * oZ], bias [Cout]
    B, C_, oZ, cells, cout = 2, 4, 3, 256, 8
    kw = dict(B=B, C=C_, oZ=oZ, cells=cells, Cout=cout, density_mode=1, voxel_output=torch.zeros(B, C_, oZ, cells),
              voxel_density=torch.zeros(B, 1, oZ, cells), weight=torch.zeros(cout, C_ * oZ), bias=torch.zeros(cout),
              out=torch.zeros(B, cout, cells), stream=None)
    assert guard.vamp_gate_conv1x1_forward(*kw.values()) == 0
    assert _violation(guard, "vamp_gate_conv1x1_forward", kw, bias=torch.zeros(cout + 1)).parameter == "bias"
    assert _violation(guard, "vamp_gate_conv1x1_forward", kw, weight=torch.zeros(C_ * oZ, cout).t()).parameter == "weight"
    assert guard.vamp_gate_conv1x1_forward(*dict(kw, bias=None).values()) == 0                # NULL is the library's business
