"""The stride-2 3x3x3 convolutions of the 3-D UNet on the 16-bit matrix cores (vampire_amd/csrc/conv3d_bf16_s2.hip;
Hourglass3D.conv1 / conv3 under a 16-bit autocast): forward, data gradient and weight gradient against
F.conv3d(x, w, stride=2, padding=1) in float64 on the CPU on the same 16-bit-rounded operands, bf16 and fp16, over the
smallest shapes that reach every branch of the three kernels; the weight gradient's repeatability, selective
gradients, misaligned views; the module path (`SWITCHES.conv3d_s2`) against the switch-off path and its routing.

The CPU tests map the cases through a Python mirror of the launchers' host-side plan and fail with the name of any
path no case reaches, compare the mirror with the library's own host answers, and pin the refusals of the entry
points and of the wrapper."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

from vampire_amd import _capi
from test_hip_parity import close, dev  # noqa: F401  (dev: the module-scoped device fixture)

F64 = torch.float64
BF16, FP16 = torch.bfloat16, torch.float16
DT_NAME = {BF16: "bf16", FP16: "fp16"}
gpu = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------ the bars
# The project's 16-bit convolution bars (tests/test_hip_parity.py::test_conv3d_bf16_matches_torch, restated in
# tests/test_layer_ops_sweep.py): one 16-bit rounding of the result on top of fp32 accumulation -- and a stride-2
# element sums fewer terms than a stride-1 one.
S2_OUT = dict(atol=1e-3, rtol=2.0 ** -8)
S2_GIN = dict(atol=1e-3, rtol=2.0 ** -8)
S2_GW = dict(atol=1e-6, rtol=2.0 ** -7, scale="max")
# A case whose fp32 arithmetic alone exceeds a bar would get max(bar, 4 x the error of fp32 aten on the CPU against
# float64) as its atol, the measured error written next to it: {(case, what): (measured, atol)}.  None needs it: the
# largest fp32-aten error over the cases below (both dtypes) is 3.5e-6 (out), 7.3e-7 (grad_in) and 1.2e-4 = 4.8e-7 of
# max |grad_weight| (grad_weight), far inside the bars.
MEASURED = {}


class Compare:
    """Every comparison of a case through test_hip_parity.close, each figure printed before anything asserts; the
    failures of the whole case are raised together at the end."""

    def __init__(self, case):
        self.case, self.failed = case, []

    def __call__(self, got, ref, bar, what):
        bar = dict(bar)
        if (self.case, what) in MEASURED:
            bar["atol"] = max(bar["atol"], MEASURED[(self.case, what)][1])
        assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
        g, r = got.detach().cpu().double(), ref.detach().cpu().double()
        err = float((g - r).abs().max()) if g.numel() else 0.0
        print(f"[conv3d_s2:{self.case}] {what}: max err {err:.3e}, max |ref| {float(r.abs().max()):.3e}, bar {bar}")
        assert bool(torch.isfinite(g).all()), f"{what}: non-finite values"
        try:
            close(got, ref.float(), what=what, **bar)
        except AssertionError as e:
            self.failed.append(str(e))

    def done(self):
        assert not self.failed, f"conv3d_s2[{self.case}]: " + "; ".join(self.failed)


def offset_view(t, dev):
    """t's values in device memory that starts one element past an allocation's first byte."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


# =====================================================================================================================
# the mirror of the host-side plan (conv3d_bf16_s2.hip: *_supported, *_workspace_bytes, launch_fwd / dgrad / wgrad)
# =====================================================================================================================
I31 = 0x7fffffff
S2_WGS = 512                                  # kWgradWgs
FWD_TX, FWD_HX = 32, 66                       # kFwdTX, kFwdHX
DG_TY, DG_TX, DG_HX = 4, 64, 34               # kDgTY, kDgTX, kDgHX
FWD_WGS, DG_WGS = 256, 512                    # kFwdWgs, kDgWgs: persistent grids, one / two workgroups per CU


def cdiv(a, b):
    return -(-a // b)


def tile_ch(c):
    return 16 if c <= 16 else 32


def osz(n):
    return (n - 1) // 2 + 1


def s2_supported(B, cin, cout, Z, Y, X):
    return int(1 <= cin <= 32 and 1 <= cout <= 32 and B > 0 and Z > 0 and Y > 0 and X >= 8 and X % 4 == 0
               and Z * Y * X * 32 * 2 < I31)


def s2_workspace(B, cin, cout, Z, Y, X):
    return S2_WGS * 27 * tile_ch(cin) * tile_ch(cout) * 4 if s2_supported(B, cin, cout, Z, Y, X) else 0


def s2_plan(B, cin, cout, Z, Y, X):
    Zo, Yo, Xo = osz(Z), osz(Y), osz(X)
    tin, tout = tile_ch(cin), tile_ch(cout)
    # forward: cin tile 16 -> 4 rows, a wave owns two N tiles; 32 -> 2 rows, a wave owns one of the two
    ty, nnw = (4, 2) if tin == 16 else (2, 1)
    tiles_x = cdiv(Xo, FWD_TX)
    fwd_nnt = tuple(max(0, min(nnw, cdiv(Xo - tx * FWD_TX - n0 * 16, 16)))
                    for tx in range(tiles_x) for n0 in ((0,) if tin == 16 else (0, 1)))
    fwd_lds = 28 * tout * tin * 2 + 3 * (2 * ty + 1) * FWD_HX * (tin * 2 + 16)
    fwd_tiles = B * Zo * cdiv(Yo, ty) * tiles_x
    # data gradient: K tile = cout's, M tile = cin's; (even, odd) N-tile pairs per 64-wide x tile
    dg_pairs = tuple(min(2, cdiv(X - tx * DG_TX, 32)) for tx in range(cdiv(X, DG_TX)))
    dg_lds = 28 * tin * tout * 2 + 2 * (DG_TY // 2 + 1) * DG_HX * (tout * 2 + 16)
    dg_tiles = B * Z * cdiv(Y, DG_TY) * cdiv(X, DG_TX)
    return dict(out=(Zo, Yo, Xo), tile=(tin, tout), fwd_nnt=fwd_nnt, fwd_lds=fwd_lds, fwd_tiles=fwd_tiles,
                fwd_grid=FWD_WGS, dg_pairs=dg_pairs, dg_lds=dg_lds, dg_tiles=dg_tiles, dg_grid=DG_WGS,
                align=16 if X % 16 == 0 else (8 if X % 8 == 0 else 4), rows=B * Zo * Yo,
                parity={(z & 1, y & 1, x & 1) for z in range(min(Z, 2)) for y in range(min(Y, 2)) for x in range(2)})


# ---- name -> (B, cin, cout, (Z, Y, X)); the tiles are at most 64 wide, so Xo = 70 needs no widening
S2_CASES = {
    "all-minimal": (1, 16, 32, (1, 1, 8)),
    "xo6-odd-y-b2": (2, 16, 16, (2, 3, 12)),
    "odd-zy-32to32": (1, 32, 32, (5, 7, 16)),
    "xo70-32to16": (1, 32, 16, (4, 6, 140)),
    "tiny-conv1-4to8": (1, 4, 8, (5, 16, 16)),
    "tiny-conv3-8to8": (1, 8, 8, (3, 8, 8)),
    "ch19to16": (1, 19, 16, (4, 4, 24)),
    "ch1to1": (1, 1, 1, (3, 3, 8)),
    "xo50-16to32": (1, 16, 32, (6, 10, 100)),
    "xo26-32to32": (1, 32, 32, (4, 9, 52)),
    # more tiles / rows than the persistent grids hold, with a remainder: the kernels' tile loops take a second turn
    "tiles-beyond-grids": (1, 16, 16, (33, 128, 8)),
}


def _inputs(B, cin, cout, vol, seed, dt):
    """As test_layer_ops_sweep._conv_inputs: randn, weights x 0.05, a seeded generator; the upstream gradient has the
    output's shape."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, *vol, generator=g).to(dt)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05).to(dt)
    up = torch.randn(B, cout, *[osz(n) for n in vol], generator=g).to(dt)
    return x, w, up


def _reference(x, w, up):
    a, wa = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv3d(a, wa, stride=2, padding=1)
    ref.backward(up.double())
    return ref.detach(), a.grad, wa.grad


_REFS = {}


def _case(name, dt, seed=4):
    """Inputs and float64 reference of a case, computed once and shared (never modified)."""
    key = (name, dt, seed)
    if key not in _REFS:
        B, cin, cout, vol = S2_CASES[name]
        x, w, up = _inputs(B, cin, cout, vol, seed, dt)
        _REFS[key] = (x, w, up) + _reference(x, w, up)
    return _REFS[key]


def _run(cmp, x, w, up, refs, grads, dev, put=lambda t, dev: t.to(dev)):
    from vampire_amd.ops import conv3d_bf16_stride2
    ref, gx, gw = refs
    b = put(x, dev).requires_grad_("x" in grads)
    wb = put(w, dev).requires_grad_("w" in grads)
    out = conv3d_bf16_stride2(b, wb)
    assert out.dtype == x.dtype
    cmp(out, ref, S2_OUT, "out")
    out.backward(put(up, dev))
    if "x" in grads:
        assert b.grad.dtype == x.dtype
        cmp(b.grad, gx, S2_GIN, "grad_in")
    else:
        assert b.grad is None
    if "w" in grads:
        assert wb.grad.dtype == w.dtype
        cmp(wb.grad, gw, S2_GW, "grad_weight")
    else:
        assert wb.grad is None
    cmp.done()


# =====================================================================================================================
# GPU
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(S2_CASES))
def test_conv3d_stride2(dev, name, dt):
    """Output, data gradient and weight gradient against F.conv3d(stride=2, padding=1) in float64."""
    from vampire_amd.ops import conv3d_bf16_stride2_supported
    x, w, up, *refs = _case(name, dt)
    assert conv3d_bf16_stride2_supported(x.to(dev), w.to(dev), (2, 2, 2), (1, 1, 1), None)
    _run(Compare(f"{name}-{DT_NAME[dt]}"), x, w, up, refs, "xw", dev)


@gpu
def test_weight_gradient_is_repeatable(dev):
    """Per-workgroup partials summed in a fixed order: two runs of one case give the same bits."""
    from vampire_amd.ops import conv3d_bf16_stride2
    x, w, up, *_ = _case("xo50-16to32", BF16)
    grads = []
    for _ in range(2):
        wb = w.to(dev).requires_grad_(True)
        conv3d_bf16_stride2(x.to(dev), wb).backward(up.to(dev))
        grads.append(wb.grad.clone())
    assert torch.equal(grads[0], grads[1])


@gpu
@pytest.mark.parametrize("grads", ["x", "w"])
def test_only_the_requested_gradient_is_computed(dev, monkeypatch, grads):
    """needs_input_grad with x only and with w only: the other entry point is not called, the other .grad stays None."""
    log = []
    lib = _capi.load()

    class Rec:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if "_s2_" not in name:
                return fn

            def call(*a):
                log.append(name)
                return fn(*a)
            return call

    via = _capi.checked(Rec())
    monkeypatch.setattr(_capi, "checked", lambda through=None: via)
    x, w, up, *refs = _case("xo6-odd-y-b2", BF16)
    _run(Compare(f"only-{grads}"), x, w, up, refs, grads, dev)
    assert ("vamp_conv3d_half_s2_backward_data" in log) == (grads == "x"), log
    assert ("vamp_conv3d_half_s2_backward_weight" in log) == (grads == "w"), log


@gpu
@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
def test_misaligned_views(dev, dt):
    """Operands one element (2 bytes) past an allocation's start: the wrapper's guard copies them; the results are
    those of aligned tensors."""
    x, w, up, *refs = _case("xo6-odd-y-b2", dt)
    _run(Compare(f"misaligned-{DT_NAME[dt]}"), x, w, up, refs, "xw", dev, put=offset_view)


# --------------------------------------------------------------------------------------------------------- the module
def _unet_run(net, x, up, dt16):
    """Output, input gradient and parameter gradients of one forward + backward, under a `dt16` autocast or (None)
    plain; as float64 CPU tensors."""
    net.zero_grad(set_to_none=True)
    a = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dt16, enabled=dt16 is not None):
        out = net(a)
    out.backward(up.to(out.dtype))
    res = {"out": out.detach(), "grad_in": a.grad}
    res.update({f"grad {n}": p.grad for n, p in net.named_parameters()})
    return {k: v.detach().cpu().double() for k, v in res.items()}


@gpu
@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
def test_unet_matches_the_switch_off_path(dev, monkeypatch, dt):
    """Unet3D(16, 16) under a 16-bit autocast with the stride-2 layers on the HIP kernels and with them in MIOpen, both
    against the same network in float64 on the CPU: the error of every tensor with the switch on is at most twice the
    switch-off error (room for another summation order, the project's usual margin) + 1e-6 of the tensor's largest
    magnitude."""
    from vampire_amd import backbone
    torch.manual_seed(3)
    net = backbone.Unet3D(16, 16)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 16, 8, 24, 40, generator=g)
    up = torch.randn(2, 16, 8, 24, 40, generator=g)
    ref = _unet_run(net.double(), x.double(), up.double(), None)
    net = net.float().to(dev)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d", True)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d_min_voxels", 0)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(backbone.SWITCHES, "conv3d_s2", on)
        res[on] = _unet_run(net, x.to(dev), up.to(dev), dt)
    assert set(res[True]) == set(ref) and len(ref) == 2 + 13
    failed = []
    for k, r in ref.items():
        e_on, e_off = float((res[True][k] - r).abs().max()), float((res[False][k] - r).abs().max())
        lim = 2 * e_off + 1e-6 * float(r.abs().max())
        print(f"[unet-{DT_NAME[dt]}] {k}: err on {e_on:.3e}, off {e_off:.3e}, max |ref| {float(r.abs().max()):.3e}, lim {lim:.3e}")
        if not e_on <= lim:
            failed.append(f"{k}: {e_on:.3e} > {lim:.3e}")
    assert not failed, "; ".join(failed)


@gpu
def test_unet_routing(dev, monkeypatch):
    """One Unet3D forward + backward under autocast calls each stride-2 entry point four times (conv1 and conv3 of the
    two hourglasses) with the switch on, never with it off, never outside autocast."""
    from vampire_amd import backbone
    log = []
    lib = _capi.load()

    class Rec:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("vamp_conv3d_half_s2_") or name.endswith(("_supported", "_bytes")):
                return fn

            def call(*a):
                log.append(name)
                return fn(*a)
            return call

    via = _capi.checked(Rec())
    monkeypatch.setattr(_capi, "checked", lambda through=None: via)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d", True)
    torch.manual_seed(3)
    net = backbone.Unet3D(16, 16).to(dev)
    x, up = torch.randn(1, 16, 4, 8, 16, device=dev), torch.ones(1, 16, 4, 8, 16, device=dev)
    names = [f"vamp_conv3d_half_s2_{n}" for n in ("forward", "backward_data", "backward_weight")]

    def counts(on, dt16):
        log.clear()
        monkeypatch.setattr(backbone.SWITCHES, "conv3d_s2", on)
        _unet_run(net, x, up, dt16)
        return [log.count(n) for n in names]

    assert isinstance(backbone.SWITCHES.conv3d_s2, bool)
    assert counts(True, BF16) == [4, 4, 4]
    assert counts(True, FP16) == [4, 4, 4]
    assert counts(False, BF16) == [0, 0, 0]
    assert counts(True, None) == [0, 0, 0]


# the entry points of each kind `layers.conv3d_kind` names (forward, data gradient, weight gradient)
KIND_ENTRIES = {None: [], "fp32": ["vamp_conv3d_forward", "vamp_conv3d_backward_data", "vamp_conv3d_backward_weight"],
                "half": [f"vamp_conv3d_half_{n}" for n in ("forward", "backward_data", "backward_weight")],
                "half_s2": [f"vamp_conv3d_half_s2_{n}" for n in ("forward", "backward_data", "backward_weight")]}


@gpu
def test_layers_and_heads_call_the_kind_conv3d_kind_names(dev, monkeypatch):
    """One forward + backward of a `_Conv3` layer at 1x16x4x8x16 (stride 1 and 2; plain, under a bf16 autocast, and
    under it with the stride-2 switch off) and of the fused heads (plain and under autocast): the convolution entry
    points recorded are exactly the three of the kind `conv3d_kind` names for the case, none where it names None."""
    from types import SimpleNamespace
    from torch import nn
    from vampire_amd import backbone
    from vampire_amd.layers import conv3d_kind
    log = []
    lib = _capi.load()

    class Rec:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith("vamp_conv3d_") or name.endswith(("_supported", "_bytes")):
                return fn

            def call(*a):
                log.append(name)
                return fn(*a)
            return call

    via = _capi.checked(Rec())
    monkeypatch.setattr(_capi, "checked", lambda through=None: via)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d", True)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d_min_voxels", 0)
    torch.manual_seed(5)
    x = torch.randn(1, 16, 4, 8, 16, device=dev)

    def check(run, w_shape, stride, dt16, s2, want):
        monkeypatch.setattr(backbone.SWITCHES, "conv3d_s2", s2)
        kind = conv3d_kind(tuple(x.shape), w_shape, torch.float32, torch.float32, True, (stride,) * 3, (1, 1, 1), False,
                           autocast=dt16, min_voxels=0, stride2=s2)
        assert kind == want, (stride, dt16, s2, kind)
        log.clear()
        a = x.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=dt16, enabled=dt16 is not None):
            outs = run(a)
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])
        assert a.grad is not None and a.grad.shape == x.shape
        assert sorted(log) == sorted(KIND_ENTRIES[kind]), (stride, dt16, s2, kind, log)

    for stride, dt16, s2, want in ((1, None, True, "fp32"), (1, BF16, True, "half"), (1, BF16, False, "half"),
                                   (2, None, True, None), (2, BF16, True, "half_s2"), (2, BF16, False, None)):
        layer = backbone._conv3(16, 32, stride).to(dev)
        check(lambda a: (layer(a),), (32, 16, 3, 3, 3), stride, dt16, s2, want)
        assert layer.weight.grad is not None and layer.weight.grad.dtype == torch.float32

    heads = SimpleNamespace(num_classes=4, density_conv=nn.Conv3d(16, 1, 3, 1, 1).to(dev),
                            seg_conv=nn.Conv3d(16, 4, 3, 1, 1).to(dev),
                            rgb_conv=nn.Sequential(nn.Conv3d(16, 3, 3, 1, 1), nn.Sigmoid()).to(dev))
    for dt16, want in ((None, "fp32"), (BF16, "half")):
        check(lambda a: backbone.BaseVAMPIRE2._heads(heads, a), (32, 16, 3, 3, 3), 1, dt16, True, want)
        assert heads.seg_conv.weight.grad is not None


# =====================================================================================================================
# CPU
# =====================================================================================================================
def test_cases_reach_every_path():
    reached = set()
    for name, (B, cin, cout, (Z, Y, X)) in S2_CASES.items():
        assert s2_supported(B, cin, cout, Z, Y, X), name
        p = s2_plan(B, cin, cout, Z, Y, X)
        tin, tout = p["tile"]
        reached |= {f"tile{tin}to{tout}", f"align{p['align']}"}
        reached |= {k for k, (n, g) in (("fwd-tiles>grid", (p["fwd_tiles"], FWD_WGS)), ("dgrad-tiles>grid", (p["dg_tiles"], DG_WGS)),
                                        ("wgrad-rows>grid", (p["rows"], S2_WGS))) if n > g and n % g}
        reached |= {f"fwd-cin{tin}-nnt{n}" for n in p["fwd_nnt"]} | {f"dgrad-pairs{n}" for n in p["dg_pairs"]}
        reached |= {f"parity{z}{y}{x}" for z, y, x in p["parity"]}
        if len(p["dg_pairs"]) > 1 and p["dg_pairs"][-1] == 1:
            reached.add("dgrad-ragged-last-x-tile")
        if cdiv(p["out"][2], FWD_TX) > 1 and p["out"][2] % FWD_TX:
            reached.add("fwd-ragged-last-x-tile")
        reached |= {k for k, v in (("Z1", Z == 1), ("Y1", Y == 1), ("X8", X == 8), ("B>1", B > 1), ("odd-Z", Z % 2 == 1),
                                   ("odd-Y", Y % 2 == 1), ("Xo%4", p["out"][2] % 4 == 2), ("Y%4", Y % DG_TY != 0),
                                   ("cin<tile", cin not in (16, 32)), ("cout<tile", cout not in (16, 32))) if v}
        assert p["fwd_lds"] <= 160 * 1024 and 2 * p["dg_lds"] <= 160 * 1024, name
    required = ({f"tile{a}to{b}" for a in (16, 32) for b in (16, 32)} | {"align16", "align8", "align4"}
                | {"fwd-cin16-nnt1", "fwd-cin16-nnt2", "fwd-cin32-nnt0", "fwd-cin32-nnt1", "dgrad-pairs1", "dgrad-pairs2"}
                | {f"parity{z}{y}{x}" for z in (0, 1) for y in (0, 1) for x in (0, 1)}
                | {"dgrad-ragged-last-x-tile", "fwd-ragged-last-x-tile", "Z1", "Y1", "X8", "B>1", "odd-Z", "odd-Y", "Xo%4",
                   "Y%4", "cin<tile", "cout<tile", "fwd-tiles>grid", "dgrad-tiles>grid", "wgrad-rows>grid"})
    missing = sorted(required - reached)
    assert not missing, f"stride-2 conv paths no case reaches: {missing}"
    # a size-1 axis has only the even class: "all-minimal" has the classes (0, 0, x) alone
    assert s2_plan(*S2_CASES["all-minimal"][:3], *S2_CASES["all-minimal"][3])["parity"] == {(0, 0, 0), (0, 0, 1)}
    # the cin = 32 forward tile and its weight image share the LDS; the UNet's shapes are supported
    assert s2_plan(1, 32, 32, 8, 100, 100)["fwd_lds"] == 28 * 32 * 32 * 2 + 15 * 66 * 80
    for d in ((1, 16, 32, 16, 200, 200), (1, 32, 32, 8, 100, 100), (1, 16, 32, 10, 128, 128), (1, 32, 32, 5, 64, 64),
              (1, 4, 8, 5, 16, 16), (1, 8, 8, 3, 8, 8)):
        assert s2_supported(*d), d


@pytest.fixture(scope="module")
def lib():
    from vampire_amd.build import build_library
    build_library(verbose=False)
    return _capi.load()


def _desc(B, cin, cout, Z, Y, X):
    d = _capi.VampConvDesc()
    d.B, d.cin, d.cout, d.Z, d.Y, d.X = B, cin, cout, Z, Y, X
    return C.byref(d)


def test_host_answers_match_the_mirror(lib):
    chans = (0, 1, 16, 17, 32, 33)
    n = 0
    for cin, cout, X, (B, Z, Y) in itertools.product(chans, chans, (4, 8, 10, 12, 200),
                                                     ((1, 1, 1), (2, 5, 7), (0, 2, 2), (1, 0, 2), (1, 2, 0), (-1, 2, 2),
                                                      (1, -3, 2), (1, 2, -2))):
        d = (B, cin, cout, Z, Y, X)
        ok, ws = lib.vamp_conv3d_half_s2_supported(_desc(*d)), lib.vamp_conv3d_half_s2_workspace_bytes(_desc(*d))
        assert ok == s2_supported(*d), d
        assert ws == s2_workspace(*d), d
        assert (ws == 0) == (ok == 0), d
        n += ok
    assert n > 50
    for X in (0, -8):
        assert lib.vamp_conv3d_half_s2_supported(_desc(1, 16, 16, 2, 2, X)) == 0
        assert lib.vamp_conv3d_half_s2_workspace_bytes(_desc(1, 16, 16, 2, 2, X)) == 0
    # the 31-bit bound on a sample's byte extent: Z Y X 64 < 2^31, the last supported volume and the first refused
    inside, past = (1, 16, 16, 4096, 1024, 8), (1, 16, 16, 4096, 1024, 12)
    assert 4096 * 1024 * 8 * 64 == 2 ** 31 and s2_supported(1, 16, 16, 4095, 1024, 8) and not s2_supported(*inside)
    for d in ((1, 16, 16, 4095, 1024, 8), inside, past):
        assert lib.vamp_conv3d_half_s2_supported(_desc(*d)) == s2_supported(*d), d
        assert lib.vamp_conv3d_half_s2_workspace_bytes(_desc(*d)) == s2_workspace(*d), d
    for name, (B, cin, cout, (Z, Y, X)) in S2_CASES.items():
        assert lib.vamp_conv3d_half_s2_supported(_desc(B, cin, cout, Z, Y, X)) == 1, name
    assert lib.vamp_conv3d_half_s2_supported(None) == 0 and lib.vamp_conv3d_half_s2_workspace_bytes(None) == 0


def test_entry_points_refuse_before_any_launch(lib):
    """A NULL tensor, dtype = VAMP_F32, an unsupported descriptor and (weight gradient) a workspace one byte short: a
    negative code and a message, with or without a GPU -- nothing is launched."""
    VAMP_F32, VAMP_BF16 = 0, 1
    good, bad = (1, 16, 32, 2, 3, 8), (1, 16, 32, 2, 3, 10)
    p = C.c_void_p(4096)             # never dereferenced: every call below returns from its argument checks
    need = lib.vamp_conv3d_half_s2_workspace_bytes(_desc(*good))
    assert need > 0

    def refused(rc, text):
        msg = lib.vamp_last_error().decode()
        assert rc < 0 and text in msg, (rc, msg)

    for name in ("forward", "backward_data"):
        fn = getattr(lib, f"vamp_conv3d_half_s2_{name}")
        for args in ((None, p, p), (p, None, p), (p, p, None)):
            refused(fn(_desc(*good), VAMP_BF16, *args, None), "NULL tensor")
        refused(fn(_desc(*good), VAMP_F32, p, p, p, None), "dtype")
        refused(fn(_desc(*bad), VAMP_BF16, p, p, p, None), "unsupported shape")
        refused(fn(None, VAMP_BF16, p, p, p, None), "unsupported shape")
    fn = lib.vamp_conv3d_half_s2_backward_weight
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        refused(fn(_desc(*good), VAMP_BF16, *args, p, need, None), "NULL tensor")
    refused(fn(_desc(*good), VAMP_F32, p, p, p, p, need, None), "dtype")
    refused(fn(_desc(*bad), VAMP_BF16, p, p, p, p, need, None), "unsupported shape")
    rc = fn(_desc(*good), VAMP_BF16, p, p, p, p, need - 1, None)
    assert rc == -2
    refused(rc, "workspace")
    refused(fn(_desc(*good), VAMP_BF16, p, p, p, None, need, None), "workspace")


def test_wrapper_refuses_cpu_and_fp32_tensors():
    from vampire_amd.ops import conv3d_bf16_stride2
    x, w = torch.zeros(1, 16, 2, 2, 8, dtype=BF16), torch.zeros(16, 16, 3, 3, 3, dtype=BF16)
    with pytest.raises(_capi.VampireHipError):
        conv3d_bf16_stride2(x, w)
    with pytest.raises(TypeError):
        conv3d_bf16_stride2(x.float(), w.float())
    with pytest.raises(TypeError):
        conv3d_bf16_stride2(x, w.to(FP16))


@gpu
def test_wrapper_refuses_fp32_device_tensors(dev):
    from vampire_amd.ops import conv3d_bf16_stride2, conv3d_bf16_stride2_supported
    x, w = torch.zeros(1, 16, 2, 2, 8, device=dev), torch.zeros(16, 16, 3, 3, 3, device=dev)
    assert not conv3d_bf16_stride2_supported(x, w, (2, 2, 2), (1, 1, 1), None)
    with pytest.raises(TypeError):
        conv3d_bf16_stride2(x, w)
    with pytest.raises(TypeError):
        conv3d_bf16_stride2(x.to(BF16), w.to(FP16))
    xb, wb = x.to(BF16), w.to(BF16)
    assert conv3d_bf16_stride2_supported(xb, wb, (2, 2, 2), (1, 1, 1), None)
    assert not conv3d_bf16_stride2_supported(xb, wb, (1, 1, 1), (1, 1, 1), None)
    assert not conv3d_bf16_stride2_supported(xb, wb, (2, 2, 2), (0, 0, 0), None)
    assert not conv3d_bf16_stride2_supported(xb[..., :6], wb, (2, 2, 2), (1, 1, 1), None)
    with pytest.raises(_capi.VampireHipError):
        conv3d_bf16_stride2(xb[..., :6].contiguous(), wb)


def test_the_stride1_rule_still_refuses_stride2():
    """`conv3d_bf16_supported` answers for the stride-1 kernels alone: callers and the sweeps' mirror rely on it."""
    from vampire_amd.ops import conv3d_bf16_supported
    x, w = torch.zeros(1, 16, 2, 2, 8, dtype=BF16), torch.zeros(16, 16, 3, 3, 3, dtype=BF16)
    assert conv3d_bf16_supported(x, w, (2, 2, 2), (1, 1, 1), None) is False


def _kind(x_shape=(1, 16, 4, 8, 16), w_shape=(32, 16, 3, 3, 3), dt=torch.float32, wdt=None, on_device=True, stride=1,
          padding=1, bias=False, **kw):
    from vampire_amd.layers import conv3d_kind
    return conv3d_kind(x_shape, w_shape, dt, dt if wdt is None else wdt, on_device, (stride,) * 3, (padding,) * 3, bias,
                       **kw)


def test_routing_table(lib):
    """Which convolution runs a layer (`layers.conv3d_kind`, what `_Conv3.forward` and `_heads` ask): the rules of the
    module path as a table, on the library's host-side shape answers."""
    V = 4 * 8 * 16
    x10, x12, c33 = (1, 16, 4, 8, 10), (1, 16, 4, 8, 12), (1, 33, 4, 8, 16)
    # the three library answers the rows rest on: X = 16 and 12 everywhere, X = 10 fp32 only, cin = 33 nowhere
    answers = lambda shape: tuple(getattr(lib, f"vamp_conv3d_{n}supported")(_desc(shape[0], shape[1], 32, *shape[2:]))  # noqa: E731
                                  for n in ("", "bf16_", "half_s2_"))
    assert answers((1, 16, 4, 8, 16)) == answers(x12) == (1, 1, 1)
    assert answers(x10) == (1, 0, 0) and answers(c33) == (0, 0, 0)
    # fp32: fp32 tensors, stride 1, no autocast of any kind, at least min_voxels voxels per channel
    assert _kind(min_voxels=0) == "fp32" and _kind() == "fp32"
    assert _kind(min_voxels=V) == "fp32" and _kind(min_voxels=V + 1) is None
    assert _kind(autocast=torch.float32) is None
    assert _kind(dt=BF16) is None and _kind(wdt=BF16) is None and _kind(dt=FP16) is None
    assert _kind(stride=2) is None and _kind(stride=2, stride2=True, min_voxels=0) is None
    # a 16-bit autocast: stride 1 before stride 2, min_voxels not applied, whatever the operands' dtypes
    for dt16 in (BF16, FP16):
        assert _kind(autocast=dt16) == "half"
        assert _kind(autocast=dt16, min_voxels=V + 1) == "half" and _kind(autocast=dt16, min_voxels=10 ** 9) == "half"
        assert _kind(autocast=dt16, dt=dt16) == "half" and _kind(autocast=dt16, stride2=False) == "half"
        assert _kind(autocast=dt16, stride=2) == "half_s2"
        assert _kind(autocast=dt16, stride=2, min_voxels=10 ** 9) == "half_s2"
        assert _kind(autocast=dt16, stride=2, stride2=False) is None
        assert _kind(x12, autocast=dt16) == "half" and _kind(x12, autocast=dt16, stride=2) == "half_s2"
        # X = 10: the fp32 kernels alone take it
        assert _kind(x10, autocast=dt16) is None and _kind(x10, autocast=dt16, stride=2) is None
    assert _kind(x10) == "fp32" and _kind(x12) == "fp32"
    # what no kernel takes, with and without autocast, at either stride
    refused = (dict(x_shape=c33, w_shape=(32, 33, 3, 3, 3)), dict(w_shape=(32, 32, 3, 3, 3)), dict(bias=True),
               dict(padding=0), dict(w_shape=(32, 16, 1, 1, 1)), dict(w_shape=(32, 16, 3, 3)), dict(x_shape=(16, 4, 8, 16)),
               dict(x_shape=(1, 1, 16, 4, 8, 16)), dict(on_device=False), dict(stride=3))
    for case, autocast, stride in itertools.product(refused, (None, BF16, FP16), (1, 2)):
        assert _kind(**{"stride": stride, **case}, autocast=autocast) is None, (case, autocast, stride)
    # the public predicates are the same rule (host tensors: refused)
    from vampire_amd.ops import conv3d_supported, conv3d_bf16_supported, conv3d_bf16_stride2_supported
    x, w = torch.zeros(1, 16, 4, 8, 16), torch.zeros(32, 16, 3, 3, 3)
    for fn, a, s in ((conv3d_supported, x, 1), (conv3d_bf16_supported, x.to(BF16), 1),
                     (conv3d_bf16_stride2_supported, x.to(BF16), 2)):
        assert fn(a, w.to(a.dtype), (s,) * 3, (1, 1, 1), None) is False
