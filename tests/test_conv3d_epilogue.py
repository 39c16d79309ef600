"""The epilogue of the 3-D convolutions (vampire_amd/csrc/conv3d_epilogue.hpp / .hip; `layers.conv3d_fused`,
`layers.conv3d_heads`, `SWITCHES.conv3d_epilogue`): y = act(conv(x, w) + bias + residual) in the convolution kernel's
store, in 1 .. 4 segments of output channels, and its backward g_z = g * act'(y) with the bias gradient.

The oracle is float64 on the CPU: F.conv3d of the exact operand values (16-bit-rounded for the half kinds), then bias,
residual and activation.  The fp32 kind is held bit for bit to the unfused sequence on the same device (`conv3d_3x3x3`,
torch's adds, F.leaky_relu); the half kinds to the project's 16-bit bars (tests/test_conv3d_stride2.py) and, for fp32
outputs, to the bound of fp32 accumulation in any order.

The CPU tests map the case table through a Python mirror of the host-side dispatch and fail with the name of any
(kind x epilogue path) no case reaches, compare the mirror with the library's own answers, and pin the refusals.

SEG_CASES drives `layers._Conv3dEpiFn.apply` with explicit segments (any first channel, order, residual, slope and
output type: what `conv3d_heads` does not expose) and with output volumes of more than one VAMP_CONV_EPI_CHUNK; those
cases hold g_z, read where the backward's entry point wrote it, bit for bit to the operator's own outputs."""
import contextlib
import ctypes as C
import functools
import os
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from vampire_amd import _capi
from test_hip_parity import close, dev  # noqa: F401  (dev: the module-scoped device fixture)
from test_conv3d_stride2 import offset_view

F64, F32, BF16, FP16 = torch.float64, torch.float32, torch.bfloat16, torch.float16
DT_NAME = {F32: "fp32", BF16: "bf16", FP16: "fp16"}
gpu = pytest.mark.gpu
NONE, LEAKY, SIGMOID = _capi.VAMP_ACT_NONE, _capi.VAMP_ACT_LEAKY_RELU, _capi.VAMP_ACT_SIGMOID
SLOPE = 0.01

# ------------------------------------------------------------------------------------------------------------ the bars
# the project's 16-bit convolution bars, as tests/test_conv3d_stride2.py states them
H_OUT = dict(atol=1e-3, rtol=2.0 ** -8)
H_GIN = dict(atol=1e-3, rtol=2.0 ** -8)
H_GW = dict(atol=1e-6, rtol=2.0 ** -7, scale="max")
# {(case, what): (measured, atol)}: a case whose fp32 arithmetic alone exceeds a bar would be listed here with the
# error of fp32 aten on the CPU against float64 next to it (the idiom of tests/test_conv3d_stride2.py).  None needs it.
MEASURED = {}
SIG_FLOOR = 2.0 ** -22          # the sigmoid's own bar: 1 / (1 + exp(-v)) in fp32, a few ulp below 1


def bar_of(case, what, bar):
    bar = dict(bar)
    if (case, what) in MEASURED:
        bar["atol"] = max(bar["atol"], MEASURED[(case, what)][1])
    return bar


def show(case, what, got, ref):
    err = float((got.detach().cpu().double() - ref.detach().cpu().double()).abs().max()) if ref.numel() else 0.0
    print(f"[conv3d_epilogue:{case}] {what}: max err {err:.3e}, max |ref| {float(ref.abs().max()):.3e}")
    return err


# =====================================================================================================================
# the cases
# =====================================================================================================================
# epilogue name -> (bias, residual, activation) of a one-segment layer
EPIS = {"none": (False, False, NONE), "bias": (True, False, NONE), "residual": (False, True, NONE),
        "leaky": (False, False, LEAKY), "residual+leaky": (False, True, LEAKY),
        "bias+residual+leaky": (True, True, LEAKY)}
# name -> (kind, B, cin, cout, (Z, Y, X)): from each kernel's tile constants the smallest volumes with a partial tile
# on every tiled axis, two tiles along x and B = 2 (the two 24 -> 8 cells at the end apart: one tile, B = 1).
#   fp32 (conv3d.hip): a wave tile is 2 .. 4 M tiles of 16 x of one row; 70 = 4 + 1 M tiles in two wave tiles, the last
#     one 6 wide, rows off a 16-byte boundary (the scalar store); 68 and 36: whole 16-byte groups (the vector store) and
#     a 4-wide last M tile; 20: one wave tile.  Every (cin, cout) pair the kind takes.  B Z Y < 16 keeps the weight
#     gradient's reduce in one slice (no float atomics between slices): bitwise repeatable.
#   half (conv3d_bf16.hip): 1 z x 4 y x 64 x tiles, 16-voxel N tiles, 16-channel M tiles.
#   half_s2 (conv3d_bf16_s2.hip): 1 zo x 4 (cin 16) or 2 (cin 32) yo x 32 xo output tiles.
LAYER_CASES = {
    "fp32-16to16-x70": ("fp32", 2, 16, 16, (2, 3, 70)),
    "fp32-16to32-x68": ("fp32", 2, 16, 32, (2, 2, 68)),
    "fp32-32to16-x20": ("fp32", 2, 32, 16, (1, 3, 20)),
    "fp32-32to32-x36": ("fp32", 2, 32, 32, (2, 2, 36)),
    "half-16to16": ("half", 2, 16, 16, (3, 5, 20)),
    "half-32to32-x68": ("half", 2, 32, 32, (2, 4, 68)),
    "s2-16to32": ("half_s2", 2, 16, 32, (3, 5, 24)),
    "s2-32to32-x72": ("half_s2", 2, 32, 32, (3, 5, 72)),
    # cin tile != cout tile in the other order than the heads' 16 -> 32 (the entry points' tile dispatch, and its swap
    # in the data gradient), at the smallest volume the 16-bit kinds take
    "half-24to8-x8": ("half", 1, 24, 8, (2, 3, 8)),
    "s2-24to8-x8": ("half_s2", 1, 24, 8, (2, 3, 8)),
}
# the three-segment heads: (kind, B, cin, cout of the weight, volume, segment channel counts).  Half: 16 -> 22 =
# 1 + 18 + 3, the boundaries at channels 1 and 19 fall inside an M tile and inside a lane's four rows.  fp32: the kind
# takes 16 or 32 output channels, so the weight is padded to 32 and the last 10 channels are computed and not stored.
HEAD_CASES = {
    "heads-half": ("half", 2, 16, 22, (2, 5, 20), (1, 18, 3)),
    "heads-fp32": ("fp32", 2, 16, 32, (2, 3, 20), (1, 18, 3)),
    "heads-s2": ("half_s2", 2, 16, 22, (3, 5, 24), (1, 18, 3)),
}
KIND_STRIDE = {"fp32": 1, "half": 1, "half_s2": 2}
KIND_DTYPES = {"fp32": (F32,), "half": (BF16, FP16), "half_s2": (BF16, FP16)}


class SegCase(NamedTuple):
    """A case driven through `layers._Conv3dEpiFn.apply` with explicit segments.  segs, in descriptor order:
    (c0, nch, activation, slope, bias, residual).  modes: the out_f32 flags it runs with (1: every output fp32 from a
    16-bit kind, with fp32 residuals).  dtypes: None = all of the kind's.  no_grad: the segments the loss leaves out."""
    kind: str
    B: int
    cin: int
    cout: int
    vol: tuple
    segs: tuple
    modes: tuple = (0,)
    dtypes: object = None
    no_grad: tuple = ()


# four segments out of channel order over a 32-channel weight: channels 16 and 29..31 lie in no segment (16 below three
# stored ones); the boundaries 3 | 17 | 20 fall inside an M tile and inside a lane's four rows, 16 | 17 on the M-tile
# boundary; two slopes; a residual with and without a bias, a bias without a residual, neither
SEG4 = ((20, 9, LEAKY, 0.2, False, True), (0, 3, NONE, 0.0, True, False), (3, 13, SIGMOID, 0.0, True, True),
        (17, 3, LEAKY, 0.01, False, False))
SEG2 = ((0, 8, LEAKY, SLOPE, False, False), (8, 8, NONE, 0.0, False, True))       # one M tile
SEG1_PARTIAL = ((5, 7, LEAKY, SLOPE, True, True),)                                 # `hit` varies per lane
HEADS3 = ((0, 1, NONE, 0.0, True, False), (1, 18, NONE, 0.0, True, False), (19, 3, SIGMOID, 0.0, True, False))
FULL16 = ((0, 16, LEAKY, SLOPE, True, True),)                                      # bias + residual + leaky
# The volumes of the segment cases are those of LAYER_CASES / HEAD_CASES above (x70: the fp32 kind's scalar store; x68:
# its 16-byte store, here with a residual).  The chunk cases are the smallest planes past VAMP_CONV_EPI_CHUNK = 4096
# voxels: 3 * 21 * 70 = 4410 = 4096 + 256 + 58 (the last chunk ends inside its second round of 256 threads),
# 4 * 17 * 64 = 4352 = 4096 + 256 (on a round), 3 * 23 * 60 = 4140 (inside the first round).  bias-65: B * nchunks =
# 65 partials per channel, one more than the finishing kernel's 64 lanes.
SEG_CASES = {
    "seg4-half": SegCase("half", 2, 16, 32, (2, 5, 20), SEG4, (0, 1)),
    "seg4-s2": SegCase("half_s2", 2, 16, 32, (3, 5, 24), SEG4, (0, 1)),
    "seg4-fp32-x70": SegCase("fp32", 2, 16, 32, (2, 3, 70), SEG4),
    "seg4-fp32-x68": SegCase("fp32", 2, 16, 32, (2, 2, 68), SEG4),
    "seg2-half": SegCase("half", 2, 16, 16, (2, 5, 20), SEG2),
    "seg2-s2": SegCase("half_s2", 2, 16, 16, (3, 5, 24), SEG2),
    "seg2-fp32-x70": SegCase("fp32", 2, 16, 16, (2, 3, 70), SEG2),
    "seg2-fp32-x68": SegCase("fp32", 2, 16, 16, (2, 2, 68), SEG2),
    "seg1-partial-half": SegCase("half", 2, 16, 16, (2, 5, 20), SEG1_PARTIAL, (0, 1)),
    "seg1-partial-s2": SegCase("half_s2", 2, 16, 16, (3, 5, 24), SEG1_PARTIAL, (0, 1)),
    "seg1-partial-fp32": SegCase("fp32", 2, 16, 16, (2, 3, 70), SEG1_PARTIAL),
    "seg4-unused": SegCase("half", 2, 16, 32, (2, 5, 20), SEG4, (0,), (BF16,), no_grad=(1, 3)),
    "fp32-chunks": SegCase("fp32", 3, 16, 16, (3, 21, 70), FULL16),
    "fp32-chunks-round": SegCase("fp32", 2, 16, 16, (4, 17, 64), FULL16),
    "half-chunks": SegCase("half", 3, 16, 16, (3, 23, 60), FULL16),
    "s2-chunks": SegCase("half_s2", 2, 16, 16, (5, 45, 120), FULL16),
    "heads-chunks": SegCase("half", 2, 16, 22, (3, 23, 60), HEADS3, (1,), (BF16,)),
    "bias-65-fp32": SegCase("fp32", 65, 16, 16, (2, 3, 8), FULL16),
    "bias-65-half": SegCase("half", 65, 16, 16, (2, 3, 8), FULL16, (0,), (BF16,)),
    "bias-65-s2": SegCase("half_s2", 65, 16, 16, (2, 3, 8), FULL16, (0,), (BF16,)),
}
assert 3 * 21 * 70 == 4096 + 256 + 58 and 4 * 17 * 64 == 4096 + 256 and 3 * 23 * 60 == 4096 + 44


def seg_params(names=None):
    return [pytest.param(name, dt, f32, id=f"{name}-{DT_NAME[dt]}-{'f32out' if f32 else 'own'}")
            for name, c in SEG_CASES.items() if names is None or name in names
            for dt in (c.dtypes or KIND_DTYPES[c.kind]) for f32 in c.modes]
KIND_FORWARD = {"fp32": "vamp_conv3d_epilogue_forward", "half": "vamp_conv3d_half_epilogue_forward",
                "half_s2": "vamp_conv3d_half_s2_epilogue_forward"}


def out_vol(kind, vol):
    s = KIND_STRIDE[kind]
    return tuple((n - 1) // s + 1 for n in vol)


def layer_params():
    return [pytest.param(name, dt, epi, id=f"{name}-{DT_NAME[dt]}-{epi}")
            for name, c in LAYER_CASES.items() for dt in KIND_DTYPES[c[0]] for epi in EPIS]


# =====================================================================================================================
# the mirror of the host-side dispatch (conv3d_epilogue.hpp: epi_check; conv3d_epilogue.hip: the backward's plan; the
# three launchers' instantiation choice)
# =====================================================================================================================
I31 = 0x7fffffff
CHUNK = _capi.VAMP_CONV_EPI_CHUNK


def cdiv(a, b):
    return -(-a // b)


def tile_ch(c):
    return 16 if c <= 16 else 32


def kind_supported(kind, B, cin, cout, vol):
    Z, Y, X = vol
    if kind == "fp32":
        if not (B > 0 and Z > 0 and Y > 0 and X > 0 and cin in (16, 32) and cout in (16, 32)):
            return False
        xs = (cdiv(X, 4) * 4 + 4 - 4 + 31) // 32 * 32 + 4
        return (cin + cout) * X <= 24 * 512 and max((cout + 3 * cin) * xs, 4 * 9 * 256) * 4 <= 160 * 1024
    return (1 <= cin <= 32 and 1 <= cout <= 32 and B > 0 and Z > 0 and Y > 0 and X >= 8 and X % 4 == 0
            and Z * Y * X * 32 * 2 < I31)


def mirror_supported(kind, dt, B, cin, cout, vol, segs):
    """segs: [(c0, nch, act, out_f32)].  The answer of vamp_conv3d_epilogue_supported."""
    if not (kind_supported(kind, B, cin, cout, vol) and B <= 65535):
        return 0
    if not 1 <= len(segs) <= 4:
        return 0
    for i, (c0, nch, act, f32) in enumerate(segs):
        if not (c0 >= 0 and nch >= 1 and c0 + nch <= cout and act in (NONE, LEAKY, SIGMOID) and f32 in (0, 1)):
            return 0
        if f32 and kind == "fp32":
            return 0
        if f32 != segs[0][3]:
            return 0
        for a0, an, _, _ in segs[:i]:
            if not (c0 >= a0 + an or a0 >= c0 + nch):
                return 0
    return 1


def mirror_workspace(kind, B, cout, vol):
    zo, yo, xo = out_vol(kind, vol)
    return cdiv(cout * B * cdiv(zo * yo * xo, CHUNK) * 8, 256) * 256


def mirror_paths(kind, dt, B, cin, cout, vol, segs, has_bias, has_res, no_grad=()):
    """The (kind x epilogue path) pairs a case reaches: the forward instantiation, its store variants, what a segment's
    epilogue does, and the backward's plan.  no_grad: the segments whose output receives no gradient."""
    zo, yo, xo = out_vol(kind, vol)
    p = {(kind, f"tile {tile_ch(cin)}->{tile_ch(cout)}")}
    stores = []
    if kind == "fp32":
        groups = [xb for xb in range(0, cdiv(xo, 16) * 16, 4)]
        stores = sorted({"store vec4" if xo % 4 == 0 and xb + 3 < xo else "store scalar" for xb in groups if xb < xo})
        p |= {(kind, s) for s in stores}
        p.add((kind, "x tiles 2" if cdiv(cdiv(xo, 16), 4) > 1 else "x tiles 1"))
    else:
        tx = 64 if kind == "half" else 32
        p.add((kind, "x tiles 2" if cdiv(xo, tx) > 1 else "x tiles 1"))
        p.add((kind, f"dtype {DT_NAME[dt]}"))
    held = sum(n for _, n, _, _ in segs)
    p.add((kind, "segments 1" if len(segs) == 1 else f"segments {len(segs)}"))
    if held < cout:
        p.add((kind, "unstored channels"))
    for (c0, nch, act, f32), b, r in zip(segs, has_bias, has_res):
        p.add((kind, "bias" if b else "no bias"))
        p.add((kind, "residual" if r else "no residual"))
        p.add((kind, {NONE: "act none", LEAKY: "act leaky", SIGMOID: "act sigmoid"}[act]))
        p.add((kind, "out fp32 from 16-bit" if f32 else "out compute dtype"))
    plain = len(segs) == 1 and segs[0][2] == NONE and not any(has_bias) and not segs[0][3] and held == cout
    p.add((kind, "backward skipped" if plain else "backward pass"))
    if any(has_bias):
        p.add((kind, "bias partials"))
    # ---- the forward's segment selection (epi_store_tile's two paths; the fp32 kind's store selects per lane always)
    multi = len(segs) > 1
    more = set()
    if multi:
        if [s[0] for s in segs] != sorted(s[0] for s in segs):
            more.add("segments out of channel order")
        if any(has_res):
            more.add("multi-seg residual")
            if segs[0][3]:
                more.add("multi-seg residual fp32")         # the raw 32-bit load under OF32
        if any(s[2] == LEAKY for s in segs):
            more.add("multi-seg leaky")
        if any(has_bias) and not all(has_bias):
            more.add("multi-seg mixed bias")
        if not segs[0][3]:
            more.add("multi-seg compute dtype")
        more.add(f"segments {len(segs)}")
        # the fp32 kind has one store per 16 bytes or per element: a multi-segment path is reached per store variant
        p |= {(kind, f"{m} {s}") for m in more for s in stores}
    elif segs[0][0] > 0 or segs[0][1] < cout:
        more.add("one segment partial")
    stored = set().union(*[range(c0, c0 + n) for c0, n, _, _ in segs])
    if set(range(max(stored))) - stored:
        more.add("gap channel")
    if any(f32 and r for (_, _, _, f32), r in zip(segs, has_res)):
        more.add("out fp32 + residual")
    if no_grad:
        more.add("segment without gradient")
    # ---- the backward's chunks (conv3d_epi_bwd_kernel, conv3d_epi_bias_kernel)
    if not plain:
        plane = zo * yo * xo
        nchunks = cdiv(plane, CHUNK)
        more.add("bwd chunks 1" if nchunks == 1 else "bwd chunks 2+")
        if nchunks > 1:
            more.add("multi-seg bwd chunks 2+" if multi else "one-seg bwd chunks 2+")
            rest = plane - (nchunks - 1) * CHUNK
            more.add("bwd last chunk ends on a round" if rest % 256 == 0 else "bwd last chunk ends inside a round")
        if any(has_bias) and B * nchunks > 64:
            more.add("bias partials wrap the 64 lanes")
    return p | {(kind, m) for m in more}


def case_table():
    """Every case of this file as the mirror's arguments."""
    rows = []
    for name, (kind, B, cin, cout, vol) in LAYER_CASES.items():
        for dt in KIND_DTYPES[kind]:
            for epi, (b, r, act) in EPIS.items():
                rows.append((f"{name}-{epi}", kind, dt, B, cin, cout, vol, [(0, cout, act, 0)], [b], [r]))
    for name, (kind, B, cin, cout, vol, chans) in HEAD_CASES.items():
        for dt in KIND_DTYPES[kind]:
            f32 = int(kind != "fp32")
            segs = [(0, chans[0], NONE, f32), (chans[0], chans[1], NONE, f32),
                    (chans[0] + chans[1], chans[2], SIGMOID, f32)]
            rows.append((name, kind, dt, B, cin, cout, vol, segs, [True] * 3, [False] * 3))
    for name, c in SEG_CASES.items():
        for dt in c.dtypes or KIND_DTYPES[c.kind]:
            for f32 in c.modes:
                rows.append((name, c.kind, dt, c.B, c.cin, c.cout, c.vol, [(c0, n, act, f32) for c0, n, act, _, _, _ in c.segs],
                             [s[4] for s in c.segs], [s[5] for s in c.segs]))
    return rows


EVERY_KIND = ["x tiles 1", "x tiles 2", "segments 1", "segments 3", "bias", "no bias", "residual",
              "no residual", "act none", "act leaky", "act sigmoid", "out compute dtype", "backward skipped",
              "backward pass", "bias partials",
              # the segment selection and the backward's chunks
              "segments 2", "segments 4", "segments out of channel order", "gap channel", "multi-seg residual",
              "multi-seg leaky", "multi-seg mixed bias", "multi-seg compute dtype", "one segment partial",
              "bwd chunks 1", "bwd chunks 2+", "one-seg bwd chunks 2+", "bwd last chunk ends inside a round",
              "bias partials wrap the 64 lanes"]
# Per kind where the kind has a kernel of its own for the path (the stores); once where the code is shared and a kind
# adds nothing: the backward kernel is instantiated per dtype, not per kind (a last chunk that ends on a round and the
# three-segment heads over two chunks run on one kind), and a segment without a gradient is the wrapper's affair.
WANTED = ({(k, p) for k in KIND_STRIDE for p in EVERY_KIND}
          | {("fp32", p) for p in ("tile 16->16", "tile 16->32", "tile 32->16", "tile 32->32", "store vec4",
                                   "store scalar", "unstored channels", "bwd last chunk ends on a round")}
          | {("fp32", f"{p} {s}") for p in ("segments 2", "segments 4", "multi-seg residual", "multi-seg leaky",
                                            "multi-seg mixed bias") for s in ("store vec4", "store scalar")}
          | {(k, p) for k in ("half", "half_s2") for p in ("tile 16->32", "tile 32->16", "tile 32->32", "dtype bf16",
                                                           "dtype fp16", "out fp32 + residual",
                                                           "multi-seg residual fp32")}
          | {("half", "out fp32 from 16-bit"), ("half_s2", "out fp32 from 16-bit"), ("half", "tile 16->16"),
             ("half", "multi-seg bwd chunks 2+"), ("half", "segment without gradient")})


def reached_paths(rows):
    reached = set()
    for name, *args in rows:
        assert mirror_supported(*args[:7]) == 1, f"{name}: the mirror refuses the case"
        reached |= mirror_paths(*args, no_grad=SEG_CASES[name].no_grad if name in SEG_CASES else ())
    return reached


def test_case_table_reaches_every_path():
    missing = sorted(WANTED - reached_paths(case_table()))
    assert not missing, f"no case reaches: {missing}"


def test_every_segment_case_is_needed():
    """Without any one of the SEG_CASES the reach check fails: no case of that table is a duplicate of the others."""
    rows = case_table()
    for name in SEG_CASES:
        assert WANTED - reached_paths([r for r in rows if r[0] != name]), f"{name} reaches nothing of its own"


def _desc(B, cin, cout, vol):
    return _capi.VampConvDesc(B, cin, cout, *vol)


def _epi(segs, ptr=None, **fields):
    """An epilogue descriptor from [(c0, nch, act, out_f32)]; `ptr`: an address for the forward pointers."""
    e = _capi.VampConvEpilogue()
    e.nseg = len(segs)
    for k, (c0, nch, act, f32) in enumerate(segs[:4]):
        g = e.seg[k]
        g.c0, g.nch, g.act, g.out_f32, g.slope = c0, nch, act, f32, SLOPE
        g.out = g.grad_out = ptr
        for f, v in fields.items():
            setattr(g, f, v)
    return e


def bad_segs(cout):
    """Segment lists the contract refuses, for a layer of `cout` >= 16 output channels."""
    return {"overlap": [(0, cout - 6, NONE, 0), (cout - 7, 7, NONE, 0)],
            "outside": [(cout - 8, 9, NONE, 0)],
            "negative c0": [(-1, 4, NONE, 0)],
            "empty": [(0, 0, NONE, 0)],
            "unknown act": [(0, 16, 3, 0)],
            "out_f32 flag": [(0, 16, NONE, 2)],
            "mixed out_f32": [(0, 8, NONE, 1), (8, 8, NONE, 0)]}


def test_mirror_agrees_with_the_library():
    lib = _capi.load()
    for name, kind, dt, B, cin, cout, vol, segs, _, _ in case_table():
        d, code = _desc(B, cin, cout, vol), {F32: 0, BF16: 1, FP16: 2}[dt]
        args = (kind, dt, B, cin, cout, vol)
        assert lib.vamp_conv3d_epilogue_supported(d, KIND_STRIDE[kind], code, _epi(segs)) == mirror_supported(*args, segs) == 1, name
        assert lib.vamp_conv3d_epilogue_workspace_bytes(d, KIND_STRIDE[kind]) == mirror_workspace(kind, B, cout, vol), name
        for why, bad in bad_segs(cout).items():
            assert lib.vamp_conv3d_epilogue_supported(d, KIND_STRIDE[kind], code, _epi(bad)) == mirror_supported(*args, bad) == 0, (name, why)
        f32seg = [(0, cout, NONE, 1)]
        assert lib.vamp_conv3d_epilogue_supported(d, KIND_STRIDE[kind], code, _epi(f32seg)) == mirror_supported(*args, f32seg) == int(kind != "fp32"), name
    # shapes the kinds refuse, a stride and dtype no kind has, a chunk boundary of the workspace
    for kind, dt, shape in (("fp32", F32, (1, 8, 16, (4, 4, 4))), ("half", BF16, (1, 16, 16, (4, 4, 6))),
                            ("half_s2", FP16, (1, 16, 33, (4, 4, 8))), ("fp32", F32, (1, 16, 16, (4, 4, 400)))):
        d, code = _desc(*shape), {F32: 0, BF16: 1, FP16: 2}[dt]
        seg = [(0, min(shape[2], 16), NONE, 0)]
        assert lib.vamp_conv3d_epilogue_supported(d, KIND_STRIDE[kind], code, _epi(seg)) == mirror_supported(kind, dt, *shape, seg) == 0
    d = _desc(1, 16, 16, (4, 4, 8))
    assert lib.vamp_conv3d_epilogue_supported(d, 2, 0, _epi([(0, 16, NONE, 0)])) == 0          # fp32 has no stride 2
    assert lib.vamp_conv3d_epilogue_supported(d, 3, 1, _epi([(0, 16, NONE, 0)])) == 0
    assert lib.vamp_conv3d_epilogue_supported(d, 1, 1, None) == 0
    assert lib.vamp_conv3d_epilogue_workspace_bytes(None, 1) == 0
    assert lib.vamp_conv3d_epilogue_workspace_bytes(d, 3) == 0
    for vol in ((1, 64, 64), (1, 64, 68)):                                                     # 4096 and 4352 voxels
        assert lib.vamp_conv3d_epilogue_workspace_bytes(_desc(3, 16, 22, vol), 1) == mirror_workspace("half", 3, 22, vol)


def test_struct_layout():
    assert C.sizeof(_capi.VampConvEpiSeg) == 5 * 8 + 6 * 4
    assert C.sizeof(_capi.VampConvEpilogue) == 8 + 4 * C.sizeof(_capi.VampConvEpiSeg)


def _forward_calls(lib, d, epi, ptr):
    """The three epilogue forwards on one descriptor: (name, return code)."""
    return [("fp32", lib.vamp_conv3d_epilogue_forward(d, epi, ptr, ptr, None)),
            ("half", lib.vamp_conv3d_half_epilogue_forward(d, _capi.VAMP_BF16, epi, ptr, ptr, None)),
            ("half_s2", lib.vamp_conv3d_half_s2_epilogue_forward(d, _capi.VAMP_F16, epi, ptr, ptr, None))]


def test_refusals_return_before_any_launch():
    """Every refusal of the contract, on a machine without a GPU: the code is VAMP_EINVAL / VAMP_ENOSPC with the
    check's own message -- a call that went on to a launch would return VAMP_EHIP (or fault on the made-up address)."""
    lib = _capi.load()
    d, ptr = _desc(1, 16, 16, (2, 4, 8)), 0x10000
    ok = [(0, 16, NONE, 0)]
    msgs = {"overlap": b"segments overlap", "outside": b"segment outside", "negative c0": b"segment outside",
            "empty": b"segment outside", "unknown act": b"unknown activation", "out_f32 flag": b"out_f32 must be",
            "mixed out_f32": b"share out_f32"}
    for why, bad in bad_segs(16).items():
        for kind, rc in _forward_calls(lib, d, _epi(bad, ptr), ptr):
            assert rc == -1, (why, kind)
        assert msgs[why] in lib.vamp_last_error(), (why, lib.vamp_last_error())     # (the last call: a 16-bit kind)
        assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, _epi(bad, ptr), ptr, None, 0, None) == -1, why
    for nseg in (0, 5, -1):
        e = _epi(ok, ptr)
        e.nseg = nseg
        assert [rc for _, rc in _forward_calls(lib, d, e, ptr)] == [-1, -1, -1], nseg
        assert b"1 <= nseg <= 4" in lib.vamp_last_error()
        assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, e, ptr, None, 0, None) == -1
    # NULL required pointers: the epilogue, a segment's output, the operands, the backward's tensors
    assert [rc for _, rc in _forward_calls(lib, d, None, ptr)] == [-1, -1, -1]
    assert [rc for _, rc in _forward_calls(lib, d, _epi(ok, None), ptr)] == [-1, -1, -1]
    assert b"NULL segment output" in lib.vamp_last_error()
    assert [rc for _, rc in _forward_calls(lib, d, _epi(ok, ptr), None)] == [-1, -1, -1]
    assert b"NULL tensor" in lib.vamp_last_error()
    assert [rc for _, rc in _forward_calls(lib, None, _epi(ok, ptr), ptr)] == [-1, -1, -1]
    assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, _epi(ok, None), ptr, None, 0, None) == -1
    assert b"NULL segment gradient" in lib.vamp_last_error()
    assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, _epi(ok, ptr), None, None, 0, None) == -1
    assert b"NULL grad_z" in lib.vamp_last_error()
    assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, _epi([(0, 16, LEAKY, 0)], ptr, out=None), ptr, None, 0, None) == -1
    assert b"needs the segment's output" in lib.vamp_last_error()
    # a tensor off a 16-byte boundary (the wrappers copy such views first)
    assert [rc for _, rc in _forward_calls(lib, d, _epi(ok, ptr + 4), ptr)] == [-1, -1, -1]
    assert b"16-byte boundary" in lib.vamp_last_error()
    assert [rc for _, rc in _forward_calls(lib, d, _epi(ok, ptr), ptr + 8)] == [-1, -1, -1]
    assert b"in / weight must start on a 16-byte boundary" in lib.vamp_last_error()
    # a *_supported question leaves the last error's text alone, and the backward keeps its own
    assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, _epi([(0, 16, 3, 0)], ptr), ptr, None, 0, None) == -1
    assert b"vamp_conv3d_epilogue_backward" in lib.vamp_last_error() and b"unknown activation" in lib.vamp_last_error()
    assert lib.vamp_conv3d_epilogue_supported(d, 1, 0, _epi([(8, 9, NONE, 0)])) == 0
    assert lib.vamp_conv3d_epilogue_supported(_desc(1, 8, 16, (2, 4, 8)), 1, 0, _epi(ok)) == 0
    assert b"vamp_conv3d_epilogue_backward" in lib.vamp_last_error() and b"unknown activation" in lib.vamp_last_error()
    # an fp32 output from the fp32 kind's "other dtype" slot
    f32seg = [(0, 16, NONE, 1)]
    assert lib.vamp_conv3d_epilogue_forward(d, _epi(f32seg, ptr), ptr, ptr, None) == -1
    assert b"out_f32 is for the 16-bit kinds" in lib.vamp_last_error()
    assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, _epi(f32seg, ptr), ptr, None, 0, None) == -1
    # dtypes and strides no kind has
    assert lib.vamp_conv3d_half_epilogue_forward(d, _capi.VAMP_F32, _epi(ok, ptr), ptr, ptr, None) == -1
    assert lib.vamp_conv3d_half_s2_epilogue_forward(d, 7, _epi(ok, ptr), ptr, ptr, None) == -1
    assert lib.vamp_conv3d_epilogue_backward(d, 1, 7, _epi(ok, ptr), ptr, None, 0, None) == -1
    assert lib.vamp_conv3d_epilogue_backward(d, 2, 0, _epi(ok, ptr), ptr, None, 0, None) == -1
    # shapes the kinds refuse
    assert lib.vamp_conv3d_epilogue_forward(_desc(1, 8, 16, (2, 4, 8)), _epi(ok, ptr), ptr, ptr, None) == -1
    assert lib.vamp_conv3d_half_epilogue_forward(_desc(1, 16, 16, (2, 4, 6)), 1, _epi(ok, ptr), ptr, ptr, None) == -1
    # a workspace that is too small (only asked for with a bias gradient)
    need = lib.vamp_conv3d_epilogue_workspace_bytes(d, 1)
    assert need == 256 == mirror_workspace("fp32", 1, 16, (2, 4, 8))
    e = _epi(ok, ptr, grad_bias=ptr)
    assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, e, ptr, ptr, need - 1, None) == -2
    assert b"workspace" in lib.vamp_last_error()
    assert lib.vamp_conv3d_epilogue_backward(d, 1, 0, e, ptr, None, need, None) == -2


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    from vampire_amd.layers import HeadSegment, conv3d_fused, conv3d_heads
    x, w = torch.zeros(1, 16, 2, 4, 8), torch.zeros(16, 16, 3, 3, 3)
    with pytest.raises(_capi.VampireHipError, match="no CPU fallback"):
        conv3d_fused(x, w, act="leaky_relu")
    with pytest.raises(_capi.VampireHipError, match="no CPU fallback"):
        conv3d_heads(x, w, [HeadSegment(16)])
    with pytest.raises(ValueError, match="act must be"):
        conv3d_fused(x, w, act="relu")
    with pytest.raises(ValueError, match="1 to 4 segments"):
        conv3d_heads(x, w, [HeadSegment(1)] * 5)


@gpu
def test_wrappers_refuse_wrong_dtypes_and_shapes(dev):
    from vampire_amd.layers import HeadSegment, conv3d_fused, conv3d_heads
    x, w = torch.zeros(1, 16, 2, 4, 8, device=dev), torch.zeros(16, 16, 3, 3, 3, device=dev)
    with pytest.raises(TypeError, match="must share"):
        conv3d_fused(x, w.to(BF16))
    with pytest.raises(TypeError, match="must share"):
        conv3d_fused(x.double(), w.double())
    with pytest.raises(_capi.VampireHipError, match="no HIP convolution"):
        conv3d_fused(x, w, stride=2)                                   # fp32 has no stride-2 kernel: no fallback
    with pytest.raises(_capi.VampireHipError, match="no HIP convolution"):
        conv3d_fused(x[:, :8], w[:, :8])
    with pytest.raises(ValueError, match="bias"):
        conv3d_fused(x, w, bias=torch.zeros(15, device=dev))
    with pytest.raises(ValueError, match="residual"):
        conv3d_fused(x, w, residual=torch.zeros(1, 16, 2, 4, 4, device=dev))
    with pytest.raises(_capi.VampireHipError, match="device tensors only"):
        conv3d_fused(x, w, bias=torch.zeros(16))
    with pytest.raises(ValueError, match="segments hold"):
        conv3d_heads(x, w, [HeadSegment(10), HeadSegment(10)])
    with pytest.raises(TypeError, match="segment's dtype"):
        conv3d_heads(x, w, [HeadSegment(16, None, None, BF16)])


def test_switch_is_a_bool_and_off_by_default():
    from vampire_amd import backbone
    assert isinstance(backbone.SWITCHES.conv3d_epilogue, bool)
    assert backbone._Switches.conv3d_epilogue == (os.environ.get("VAMP_CONV3D_EPILOGUE", "0") == "1")
    if "VAMP_CONV3D_EPILOGUE" not in os.environ:
        assert backbone.SWITCHES.conv3d_epilogue is False


# =====================================================================================================================
# GPU: one layer
# =====================================================================================================================
def _act64(v, act):
    if act == LEAKY:
        return torch.where(v > 0, v, v * SLOPE)
    return torch.sigmoid(v) if act == SIGMOID else v


@functools.lru_cache(maxsize=None)
def _operands(name, dt):
    """The operands of a case, rounded to its dtype, on the CPU: x, w, bias (fp32), residual, the upstream gradient;
    and the float64 convolution of the rounded values with its absolute-value companion sum |w x|."""
    kind, B, cin, cout, vol = (LAYER_CASES.get(name) or HEAD_CASES.get(name) or SEG_CASES[name])[:5]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    ov = out_vol(kind, vol)
    x = torch.randn(B, cin, *vol, generator=g).to(dt)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (27 * cin)) ** 0.5).to(dt)
    bias = torch.randn(cout, generator=g)
    res = torch.randn(B, cout, *ov, generator=g).to(dt)
    up = torch.randn(B, cout, *ov, generator=g).to(dt)
    s = KIND_STRIDE[kind]
    conv = F.conv3d(x.double(), w.double(), stride=s, padding=1)
    absum = F.conv3d(x.double().abs(), w.double().abs(), stride=s, padding=1)
    return x, w, bias, res, up, conv, absum


def _oracle(name, dt, has_bias, has_res, act):
    """float64: out, grad_x, grad_w, grad_bias, grad_residual of sum(out * up)."""
    kind = LAYER_CASES[name][0]
    x, w, bias, res, up, _, _ = _operands(name, dt)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    bd, rd = bias.double().requires_grad_(True), res.double().requires_grad_(True)
    v = F.conv3d(xd, wd, stride=KIND_STRIDE[kind], padding=1)
    if has_bias:
        v = v + bd.view(1, -1, 1, 1, 1)
    if has_res:
        v = v + rd
    out = _act64(v, act)
    out.backward(up.double())
    return out.detach(), xd.grad, wd.grad, bd.grad, rd.grad


def _run_fused(name, dt, epi, dev, put=lambda t, dev: t.to(dev), grads="xwbr"):
    """conv3d_fused on the case's operands: (out, grad_x, grad_w, grad_bias, grad_residual) as device tensors."""
    from vampire_amd.layers import conv3d_fused
    kind = LAYER_CASES[name][0]
    has_bias, has_res, act = EPIS[epi]
    x, w, bias, res, up, _, _ = _operands(name, dt)
    xs = put(x, dev).requires_grad_("x" in grads)
    ws = put(w, dev).requires_grad_("w" in grads)
    bs = put(bias, dev).requires_grad_("b" in grads) if has_bias else None
    rs = put(res, dev).requires_grad_("r" in grads) if has_res else None
    out = conv3d_fused(xs, ws, bs, rs, {NONE: None, LEAKY: "leaky_relu"}[act], SLOPE, KIND_STRIDE[kind])
    if out.requires_grad:
        out.backward(up.to(dev))
    return out.detach(), xs.grad, ws.grad, None if bs is None else bs.grad, None if rs is None else rs.grad


def _gz_expected(out, up, act):
    """g_z from the operator's own y: aten's leaky_relu_backward on the result, or the gradient itself."""
    if act == LEAKY:
        return torch.ops.aten.leaky_relu_backward(up, out, SLOPE, True)
    return up


def _ulp32(v):
    """One fp32 ulp at |v| (v: float64 tensor)."""
    return torch.maximum(torch.abs(torch.nextafter(v.float(), torch.full_like(v.float(), float("inf"))) - v.float()).double(),
                         torch.full_like(v, 2.0 ** -149))


@gpu
@pytest.mark.parametrize("name,dt,epi", layer_params())
def test_layer_epilogues(dev, name, dt, epi):
    """Every epilogue of a one-segment layer, per kind, shape and dtype."""
    from vampire_amd.layers import conv3d_3x3x3
    kind = LAYER_CASES[name][0]
    has_bias, has_res, act = EPIS[epi]
    case = f"{name}-{DT_NAME[dt]}-{epi}"
    out, gx, gw, gb, gr = _run_fused(name, dt, epi, dev)
    x, w, bias, res, up, _, _ = _operands(name, dt)
    r_out, r_gx, r_gw, r_gb, r_gr = _oracle(name, dt, has_bias, has_res, act)
    assert out.dtype == dt and gx.dtype == dt and gw.dtype == dt and tuple(out.shape) == tuple(r_out.shape)
    failed = []

    def check(what, got, ref, bar):
        show(case, what, got, ref)
        try:
            close(got, ref.float(), what=what, **bar_of(case, what, bar))
        except AssertionError as e:
            failed.append(str(e))

    check("out", out, r_out, H_OUT)
    check("grad_x", gx, r_gx, H_GIN)
    check("grad_w", gw, r_gw, H_GW)
    # g_z, bit for bit: aten's backward of the activation on the operator's own y (the residual's gradient IS g_z)
    gz = _gz_expected(out, up.to(dev), act)
    if has_res:
        assert gr.dtype == dt and torch.equal(gr, gz), f"{case}: grad_residual is not g_z"
    if has_bias:
        want = gz.double().sum(dim=(0, 2, 3, 4)).cpu()
        err = (gb.double().cpu() - want).abs()
        print(f"[conv3d_epilogue:{case}] grad_bias: max err {float(err.max()):.3e} (one ulp {float(_ulp32(want).min()):.3e} ..)")
        assert gb.dtype == F32 and bool((err <= _ulp32(want)).all()), f"{case}: grad_bias beyond one fp32 ulp of sum(g_z)"
    if kind == "fp32":
        # the unfused sequence on the same device, bit for bit
        xs, ws = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
        rs = res.to(dev).requires_grad_(True)
        v = conv3d_3x3x3(xs, ws)
        if has_bias:
            v = v + bias.to(dev).view(1, -1, 1, 1, 1)
        if has_res:
            v = v + rs
        u_out = F.leaky_relu(v, SLOPE) if act == LEAKY else v
        u_out.backward(up.to(dev))
        for what, got, ref in (("out", out, u_out.detach()), ("grad_x", gx, xs.grad), ("grad_w", gw, ws.grad)) + (
                (("grad_residual", gr, rs.grad),) if has_res else ()):
            if not torch.equal(got, ref):
                failed.append(f"{what}: not bit-equal to the unfused sequence (max diff {float((got - ref).abs().max()):.3e})")
    assert not failed, f"{case}: " + "; ".join(failed)


def _head_segments(name, dt, bias, dev):
    from vampire_amd.layers import HeadSegment
    chans = HEAD_CASES[name][5]
    c = [0, chans[0], chans[0] + chans[1], sum(chans)]
    acts = (None, None, "sigmoid")
    return [HeadSegment(chans[k], bias[c[k]:c[k + 1]], acts[k], F32) for k in range(3)], c


@gpu
@pytest.mark.parametrize("name,dt", [pytest.param(n, dt, id=f"{n}-{DT_NAME[dt]}")
                                     for n, c in HEAD_CASES.items() for dt in KIND_DTYPES[c[0]]])
def test_three_segment_heads(dev, name, dt):
    """density / logits / rgb + sigmoid from one convolution into three fp32 tensors.  An fp32 output of a 16-bit kind
    lies within (27 cin + 4) 2^-24 (sum |w x| + |bias|) of the float64 value, the bound of fp32 accumulation in any
    order; behind the sigmoid (slope <= 1/4) a quarter of it plus the sigmoid's own 2^-22.  The fp32 kind: the plain
    segments bit-equal to the unfused sequence, the sigmoid within max(2 x the unfused error, 2^-22); gradients within
    twice the unfused sequence's own error + 1e-6 of the largest magnitude (the module tests' margin).  The bias
    gradient, every kind: within one fp32 ulp of the float64 sum of the operator's own g_z -- the upstream gradient
    itself for the two plain segments, (g (1 - y)) y in fp32 from the operator's own y behind the sigmoid."""
    from vampire_amd.layers import conv3d_3x3x3, conv3d_bf16, conv3d_bf16_stride2, conv3d_heads
    stride = KIND_STRIDE[HEAD_CASES[name][0]]
    kind, B, cin, cout, vol, chans = HEAD_CASES[name]
    case = f"{name}-{DT_NAME[dt]}"
    x, w, bias, _, up, conv, absum = _operands(name, dt)
    up = up.float()
    xs, ws = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    bs = bias.to(dev).requires_grad_(True)
    segs, c = _head_segments(name, dt, bs, dev)
    outs = conv3d_heads(xs, ws, segs, stride=stride)
    assert [tuple(o.shape) for o in outs] == [(B, n) + out_vol(kind, vol) for n in chans] and all(o.dtype == F32 for o in outs)
    torch.autograd.backward(outs, [up[:, c[k]:c[k + 1]].to(dev).contiguous() for k in range(3)])
    # float64 oracle
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), bias.double().requires_grad_(True)
    v = F.conv3d(xd, wd, stride=stride, padding=1) + bd.view(1, -1, 1, 1, 1)
    refs = [v[:, c[0]:c[1]], v[:, c[1]:c[2]], torch.sigmoid(v[:, c[2]:c[3]])]
    torch.autograd.backward(refs, [up[:, c[k]:c[k + 1]].double() for k in range(3)])
    # the unfused sequence on the device
    xu, wu, bu = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    y = {"fp32": conv3d_3x3x3, "half": conv3d_bf16, "half_s2": conv3d_bf16_stride2}[kind](xu, wu)
    yb = y + bu.view(1, -1, 1, 1, 1)
    unf = [yb[:, c[0]:c[1]], yb[:, c[1]:c[2]], torch.sigmoid(yb[:, c[2]:c[3]])]
    torch.autograd.backward(unf, [up[:, c[k]:c[k + 1]].to(dev) for k in range(3)])
    failed = []
    bound = (27 * cin + 4) * 2.0 ** -24 * (absum + bias.double().abs().view(1, -1, 1, 1, 1))
    for k, what in enumerate(("density", "logits", "rgb")):
        got, ref = outs[k].detach().cpu().double(), refs[k].detach()
        err = (got - ref).abs()
        e_unf = float((unf[k].detach().cpu().double() - ref).abs().max())
        print(f"[conv3d_epilogue:{case}] {what}: max err {float(err.max()):.3e}, unfused {e_unf:.3e}")
        if kind == "fp32":
            if k < 2:
                ok = torch.equal(outs[k].detach(), unf[k].detach())
            else:
                ok = float(err.max()) <= max(2 * e_unf, SIG_FLOOR)
        else:
            lim = bound[:, c[k]:c[k + 1]]
            ok = bool((err <= (lim if k < 2 else 0.25 * lim + SIG_FLOOR)).all())
        if not ok:
            failed.append(f"{what}: max err {float(err.max()):.3e}")
    gb_bar = dict(atol=1e-6, rtol=2.0 ** -7, scale="max")
    for what, got, ref, unfused, bar in (("grad_x", xs.grad, xd.grad, xu.grad, H_GIN), ("grad_w", ws.grad, wd.grad, wu.grad, H_GW),
                                         ("grad_bias", bs.grad, bd.grad, bu.grad, gb_bar)):
        e, e_unf = show(case, what, got, ref), float((unfused.cpu().double() - ref).abs().max())
        if kind == "fp32":
            lim = 2 * e_unf + 1e-6 * float(ref.abs().max())
            if not e <= lim:
                failed.append(f"{what}: {e:.3e} > {lim:.3e}")
        else:
            try:
                close(got, ref.float(), what=what, **bar_of(case, what, bar))
            except AssertionError as ex:
                failed.append(str(ex))
    # the bias gradient against the operator's own g_z
    gup = [up[:, c[k]:c[k + 1]].to(dev) for k in range(3)]
    y_rgb = outs[2].detach()
    gz = torch.cat([gup[0], gup[1], (gup[2] * (1.0 - y_rgb)) * y_rgb], 1)
    assert gz.dtype == F32
    want = gz.double().sum(dim=(0, 2, 3, 4)).cpu()
    gb_err = (bs.grad[:c[3]].double().cpu() - want).abs()
    print(f"[conv3d_epilogue:{case}] grad_bias vs sum(g_z): max err {float(gb_err.max()):.3e}, in ulp "
          f"{float((gb_err / _ulp32(want)).max()):.3f}")
    if not (bs.grad.dtype == F32 and bool((gb_err <= _ulp32(want)).all())):
        failed.append(f"grad_bias beyond one fp32 ulp of sum(g_z): {float((gb_err / _ulp32(want)).max()):.3f} ulp")
    if kind == "fp32":
        assert torch.equal(ws.grad[c[3]:], torch.zeros_like(ws.grad[c[3]:])), "unstored channels have no gradient"
    assert not failed, f"{case}: " + "; ".join(failed)


@gpu
@pytest.mark.parametrize("name,dt", [("fp32-16to16-x70", F32), ("half-16to16", BF16), ("s2-16to32", FP16)])
def test_sigmoid_layer(dev, name, dt):
    """A one-segment layer behind a sigmoid: within max(2 x the unfused sequence's own error against the oracle,
    2^-22) for fp32; the 16-bit kinds round the result once more, to the 16-bit output bar."""
    from vampire_amd.layers import _Conv3dFn, conv3d_fused
    kind = LAYER_CASES[name][0]
    x, w, bias, _, _, conv, _ = _operands(name, dt)
    ref = torch.sigmoid(conv + bias.double().view(1, -1, 1, 1, 1))
    out = conv3d_fused(x.to(dev), w.to(dev), bias.to(dev), None, "sigmoid", stride=KIND_STRIDE[kind])
    unf = torch.sigmoid(_Conv3dFn.apply(kind, x.to(dev), w.to(dev)).float() + bias.to(dev).view(1, -1, 1, 1, 1))
    e, e_unf = show(name, "sigmoid out", out, ref), float((unf.cpu().double() - ref).abs().max())
    print(f"[conv3d_epilogue:{name}] unfused {e_unf:.3e}")
    if kind == "fp32":
        assert e <= max(2 * e_unf, SIG_FLOOR)
    else:
        close(out, ref.float(), what="sigmoid out", **H_OUT)


# =====================================================================================================================
# GPU: explicit segments (any c0, order, residual, slope, output type) and output volumes of more than one chunk
# =====================================================================================================================
class _Keeper:
    """The library with the arguments of every vamp_conv3d_epilogue_backward call kept (grad_z is the fifth)."""

    def __init__(self, lib, kept):
        self._lib, self._kept = lib, kept

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "vamp_conv3d_epilogue_backward":
            return fn

        def call(*a):
            self._kept.append(a)
            return fn(*a)
        return call


@contextlib.contextmanager
def _kept_backward_calls():
    kept, own = [], _capi.checked
    via = own(_Keeper(_capi.load(), kept))
    _capi.checked = lambda through=None: via
    try:
        yield kept
    finally:
        _capi.checked = own


@functools.lru_cache(maxsize=None)
def _res32(name):
    """The fp32 residual of a case's fp32-output run: unit normal, not rounded to 16 bits (all 32 bits are read)."""
    c = SEG_CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 1)
    return torch.randn(c.B, c.cout, *out_vol(c.kind, c.vol), generator=g)


def _run_segments(name, dt, f32, dev):
    """`_Conv3dEpiFn.apply` on the case's operands and the backward of sum(out * up) over the segments with a gradient.
    The operator's results as device tensors, grad_z as the backward's entry point wrote it, the gradients fed in."""
    from vampire_amd.layers import _Conv3dEpiFn, _EpiSeg
    c = SEG_CASES[name]
    x, w, bias, res, up, _, _ = _operands(name, dt)
    odt, res = (F32, _res32(name)) if f32 else (dt, res)
    xs, ws = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(True)
    segs, tensors, bs, rs, gups = [], [], {}, {}, {}
    for n, (c0, nch, act, slope, has_b, has_r) in enumerate(c.segs):
        segs.append(_EpiSeg(c0, nch, act, float(slope), bool(f32), has_b, has_r))
        if has_b:
            bs[n] = bias[c0:c0 + nch].to(dev).requires_grad_(True)
            tensors.append(bs[n])
        if has_r:
            rs[n] = res[:, c0:c0 + nch].contiguous().to(dev).requires_grad_(True)
            tensors.append(rs[n])
        if n not in c.no_grad:
            gups[n] = up[:, c0:c0 + nch].to(odt).contiguous().to(dev)
    with _kept_backward_calls() as kept:
        outs = _Conv3dEpiFn.apply(c.kind, tuple(segs), xs, ws, *tensors)
        torch.autograd.backward([outs[n] for n in gups], [gups[n] for n in gups])
    assert len(kept) == 1, f"{name}: expected one epilogue backward, saw {len(kept)}"
    return dict(outs=[o.detach() for o in outs], gx=xs.grad, gw=ws.grad, gb={n: b.grad for n, b in bs.items()},
                gr={n: r.grad for n, r in rs.items()}, gz=kept[0][4], gups=gups)


def _gz_own(c, dt, f32, outs, gups, dev):
    """g_z from the operator's own outputs: the [B, cout, Zo, Yo, Xo] tensor of the compute type (rounded once; 0 in a
    channel of no segment and in a segment without a gradient), and per segment g_z in the segment's own precision
    (what its bias gradient sums: fp32 for an fp32-output segment of a 16-bit kind)."""
    full = torch.zeros((c.B, c.cout) + out_vol(c.kind, c.vol), dtype=dt, device=dev)
    own = {}
    for n, (c0, nch, act, slope, _, _) in enumerate(c.segs):
        if n not in gups:
            continue
        g, y = gups[n], outs[n]
        if act == LEAKY:
            z = torch.ops.aten.leaky_relu_backward(g, y, slope, True)
        elif act == SIGMOID:
            z = ((g.float() * (1.0 - y.float())) * y.float()).to(g.dtype)
        else:
            z = g
        own[n] = z
        full[:, c0:c0 + nch] = z.to(dt)
    return full, own


def _held(case, what, got, ref, bar, failed):
    """`close` with the fraction of the bar on record."""
    a, b = got.detach().cpu().float(), ref.detach().cpu().float()
    err = (a - b).abs()
    lim = bar["atol"] + bar["rtol"] * (b.abs().max() if bar.get("scale") == "max" else b.abs())
    print(f"[conv3d_epilogue:{case}] {what}: max err {float(err.max()):.3e}, bar {bar['atol']:g} + {bar['rtol']:g} "
          f"{'max ' if bar.get('scale') == 'max' else ''}|ref|, fraction {float((err / lim).max()):.4f}")
    if not bool((err <= lim).all()):
        failed.append(f"{what}: max err {float(err.max()):.3e} beyond the bar")


@gpu
@pytest.mark.parametrize("name,dt,f32", seg_params())
def test_segment_and_chunk_cases(dev, name, dt, f32):
    """Outputs: compute-dtype ones to the 16-bit bars; the fp32 kind bit for bit to the unfused sequence on the device
    (conv3d_3x3x3, slice, adds, F.leaky_relu), a sigmoid segment within max(2 x the unfused error, 2^-22); fp32 outputs
    of a 16-bit kind within (27 cin + 5) 2^-24 (sum |w x| + |bias| + |residual|) of the float64 value, element by
    element -- the bound of fp32 accumulation in any order with one more addend for the residual; unchanged behind
    leaky (slope <= 1), a quarter of it plus 2^-22 behind the sigmoid.  g_z bit for bit from the operator's own
    outputs, a residual's gradient its segment's slice of it (widened for an fp32 residual of a 16-bit kind), the
    weight-gradient rows of channels without a gradient exactly 0.  grad_x and grad_w against the float64 convolution
    backward of the operator's own g_z (an element whose pre-activation lies within fp32 rounding of 0 may take either
    branch of the activation: a draw, and no element is left out this way).  grad_bias within one fp32 ulp of the
    float64 sum of the operator's own g_z in the segment's precision."""
    from vampire_amd.layers import conv3d_3x3x3
    c = SEG_CASES[name]
    case = f"{name}-{DT_NAME[dt]}-{'f32out' if f32 else 'own'}"
    odt, stride = (F32 if f32 else dt), KIND_STRIDE[c.kind]
    got = _run_segments(name, dt, f32, dev)
    x, w, bias, res, up, conv, absum = _operands(name, dt)
    res = _res32(name) if f32 else res
    failed = []
    if c.kind == "fp32":
        plain = conv3d_3x3x3(x.to(dev), w.to(dev))
    for n, (c0, nch, act, slope, has_b, has_r) in enumerate(c.segs):
        ch, what = slice(c0, c0 + nch), f"out[{n}]"
        v, mag = conv[:, ch], absum[:, ch]
        if has_b:
            v, mag = v + bias[ch].double().view(1, -1, 1, 1, 1), mag + bias[ch].double().abs().view(1, -1, 1, 1, 1)
        if has_r:
            v, mag = v + res[:, ch].double(), mag + res[:, ch].double().abs()
        ref = torch.where(v > 0, v, v * slope) if act == LEAKY else torch.sigmoid(v) if act == SIGMOID else v
        out = got["outs"][n]
        assert out.dtype == odt and tuple(out.shape) == tuple(ref.shape), what
        err = (out.cpu().double() - ref).abs()
        if c.kind == "fp32":
            u = plain[:, ch]
            if has_b:
                u = u + bias[ch].to(dev).view(1, -1, 1, 1, 1)
            if has_r:
                u = u + res[:, ch].to(dev)
            u = F.leaky_relu(u, slope) if act == LEAKY else torch.sigmoid(u) if act == SIGMOID else u
            e_unf = float((u.cpu().double() - ref).abs().max())
            lim = max(2 * e_unf, SIG_FLOOR) if act == SIGMOID else 0.0
            diff = float((out - u).abs().max())
            print(f"[conv3d_epilogue:{case}] {what}: max err {float(err.max()):.3e}, unfused {e_unf:.3e}, max |fused - "
                  f"unfused| {diff:.3e}, bar {'bit-equal' if act != SIGMOID else f'{lim:.3e}'}")
            if not (float(err.max()) <= lim if act == SIGMOID else torch.equal(out, u)):
                failed.append(f"{what}: not the unfused sequence's value (max diff {diff:.3e})")
        elif f32:
            lim = (27 * c.cin + 5) * 2.0 ** -24 * mag
            lim = 0.25 * lim + SIG_FLOOR if act == SIGMOID else lim
            print(f"[conv3d_epilogue:{case}] {what}: max err {float(err.max()):.3e}, smallest bar {float(lim.min()):.3e}, "
                  f"fraction {float((err / lim).max()):.4f}")
            if not bool((err <= lim).all()):
                failed.append(f"{what}: beyond the fp32 accumulation bound (max err {float(err.max()):.3e})")
        else:
            _held(case, what, out, ref, H_OUT, failed)
    # g_z, bit for bit
    full, own = _gz_own(c, dt, f32, got["outs"], got["gups"], dev)
    gz = got["gz"]
    assert gz.dtype == dt and gz.shape == full.shape
    wrong = int((gz != full).sum())
    print(f"[conv3d_epilogue:{case}] g_z: {wrong} of {gz.numel()} elements differ from the operator's own outputs' (bar 0)")
    if wrong:
        failed.append(f"g_z: {wrong} elements differ")
    for n, g in got["gr"].items():
        c0, nch = c.segs[n][:2]
        if not (g.dtype == odt and torch.equal(g, full[:, c0:c0 + nch].to(odt))):
            failed.append(f"grad_residual[{n}] is not its segment's slice of g_z")
    live = set().union(*[range(c.segs[n][0], c.segs[n][0] + c.segs[n][1]) for n in got["gups"]])
    dead = [ch for ch in range(c.cout) if ch not in live]
    if dead and bool((got["gw"][dead] != 0).any()):
        failed.append(f"grad_w: rows of channels without a gradient are not 0 ({dead})")
    # the convolution's backward of that g_z
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    r_gx, r_gw = torch.autograd.grad(F.conv3d(xd, wd, stride=stride, padding=1), (xd, wd), full.double().cpu())
    assert got["gx"].dtype == dt and got["gw"].dtype == dt
    _held(case, "grad_x", got["gx"], r_gx, H_GIN, failed)
    _held(case, "grad_w", got["gw"], r_gw, H_GW, failed)
    # the bias gradients
    for n, gb in got["gb"].items():
        assert gb.dtype == F32 and tuple(gb.shape) == (c.segs[n][1],)
        if n in own:
            want = own[n].double().sum(dim=(0, 2, 3, 4)).cpu()
        else:
            want = torch.zeros(c.segs[n][1], dtype=F64)
        ulps = (gb.double().cpu() - want).abs() / _ulp32(want)
        print(f"[conv3d_epilogue:{case}] grad_bias[{n}] vs sum(g_z): max err {float((gb.double().cpu() - want).abs().max()):.3e}, "
              f"bar one fp32 ulp, fraction {float(ulps.max()):.3f}")
        if not bool((ulps <= 1.0).all()):
            failed.append(f"grad_bias[{n}] beyond one fp32 ulp of sum(g_z): {float(ulps.max()):.3f} ulp")
    assert not failed, f"{case}: " + "; ".join(failed)


@gpu
@pytest.mark.parametrize("name,dt,f32", [("seg4-half", BF16, 1), ("seg4-s2", FP16, 1), ("half-chunks", BF16, 0),
                                         ("bias-65-fp32", F32, 0), ("bias-65-half", BF16, 0)])
def test_segment_and_chunk_runs_are_bitwise_equal(dev, name, dt, f32):
    """Everything but the fp32 kind's weight gradient where its reduce spans slices (B Z Y >= 16: float atomics)."""
    c = SEG_CASES[name]
    a, b = _run_segments(name, dt, f32, dev), _run_segments(name, dt, f32, dev)
    pairs = [(f"out[{n}]", p, q) for n, (p, q) in enumerate(zip(a["outs"], b["outs"]))]
    pairs += [("g_z", a["gz"], b["gz"]), ("grad_x", a["gx"], b["gx"])]
    pairs += [(f"grad_bias[{n}]", a["gb"][n], b["gb"][n]) for n in a["gb"]]
    pairs += [(f"grad_residual[{n}]", a["gr"][n], b["gr"][n]) for n in a["gr"]]
    if c.kind != "fp32" or c.B * c.vol[0] * c.vol[1] < 16:
        pairs.append(("grad_w", a["gw"], b["gw"]))
    for what, p, q in pairs:
        assert torch.equal(p, q), f"{name}: {what} differs between two runs"


# =====================================================================================================================
# GPU: repeatability, selective gradients, views, graphs
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("name,dt", [("fp32-16to32-x68", F32), ("half-32to32-x68", BF16), ("s2-16to32", FP16)])
def test_two_runs_are_bitwise_equal(dev, name, dt):
    a = _run_fused(name, dt, "bias+residual+leaky", dev)
    b = _run_fused(name, dt, "bias+residual+leaky", dev)
    for what, p, q in zip(("out", "grad_x", "grad_w", "grad_bias", "g_z"), a, b):
        assert torch.equal(p, q), f"{name}: {what} differs between two runs"


class _Recorder:
    """The library with the convolution entry points' calls logged (size and *_supported questions aside)."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("vamp_conv3d_") or name.endswith(("_supported", "_bytes")):
            return fn

        def call(*a):
            self._log.append(name)
            return fn(*a)
        return call


def _record(monkeypatch):
    log = []
    via = _capi.checked(_Recorder(_capi.load(), log))
    monkeypatch.setattr(_capi, "checked", lambda through=None: via)
    return log


@gpu
@pytest.mark.parametrize("grads,epi,want", [
    ("x", "bias+residual+leaky", ["epilogue_backward", "backward_data"]),
    ("w", "bias+residual+leaky", ["epilogue_backward", "backward_weight"]),
    ("b", "bias+residual+leaky", ["epilogue_backward"]),
    ("r", "bias+residual+leaky", ["epilogue_backward"]),
    ("x", "residual", ["backward_data"]),                  # no activation, no bias, one segment: the pass is skipped
    ("r", "residual", []),
    ("xw", "bias", ["backward_data", "backward_weight"]),  # a bias that wants no gradient does not bring the pass back
    ("", "leaky", []),
])
def test_only_the_requested_gradients_are_computed(dev, monkeypatch, grads, epi, want):
    log = _record(monkeypatch)
    out, gx, gw, gb, gr = _run_fused("half-16to16", BF16, epi, dev, grads=grads)
    assert log[0] == "vamp_conv3d_half_epilogue_forward"
    got = sorted(n.replace("vamp_conv3d_half_", "").replace("vamp_conv3d_", "") for n in log[1:])
    assert got == sorted(want), log
    for ch, g in zip("xwbr", (gx, gw, gb, gr)):
        assert (g is not None) == (ch in grads and (ch not in "br" or EPIS[epi]["br".index(ch)])), (ch, grads)
    if grads == "r":
        assert torch.equal(gr, _gz_expected(out, _operands("half-16to16", BF16)[4].to(dev), EPIS[epi][2]))


@gpu
@pytest.mark.parametrize("name,dt", [("fp32-16to16-x70", F32), ("half-16to16", FP16), ("s2-16to32", BF16)])
def test_misaligned_views(dev, name, dt):
    """Operands one element past an allocation's start: `_aligned` copies them; the values are those of aligned ones."""
    a = _run_fused(name, dt, "bias+residual+leaky", dev)
    b = _run_fused(name, dt, "bias+residual+leaky", dev, put=offset_view)
    for what, p, q in zip(("out", "grad_x", "grad_w", "grad_bias", "g_z"), a, b):
        assert torch.equal(p, q), f"{name}: {what} differs for views off a 16-byte boundary"


@gpu
@pytest.mark.parametrize("name,dt", [("fp32-16to16-x70", F32), ("half-16to16", BF16)])
def test_graph_replay_matches_eager(dev, name, dt):
    """One forward + backward of a fused layer captured on one stream (every workspace allocated by the warm-up runs on
    that stream) replays to the eager result after the input changed."""
    from vampire_amd.layers import conv3d_fused
    x, w, bias, res, up, _, _ = _operands(name, dt)
    sx = x.to(dev).requires_grad_(True)
    sw, sb = w.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    sr, sup = res.to(dev).requires_grad_(True), up.to(dev)
    leaves = (sx, sw, sb, sr)

    def step():
        out = conv3d_fused(sx, sw, sb, sr, "leaky_relu", SLOPE)
        return out, torch.autograd.grad(out, leaves, sup)

    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        g_out, g_grads = step()
    with torch.no_grad():
        sx.copy_(torch.flip(sx, dims=(-1,)) * 0.5)
    graph.replay()
    torch.cuda.synchronize(dev)
    e_out, e_grads = step()
    assert torch.equal(g_out, e_out)
    for what, p, q in zip(("grad_x", "grad_w", "grad_bias", "grad_residual"), g_grads, e_grads):
        assert torch.equal(p, q), f"{name}: replayed {what} differs from eager"


# =====================================================================================================================
# GPU: the module
# =====================================================================================================================
def _unet_run(net, x, up, dt16):
    net.zero_grad(set_to_none=True)
    a = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dt16, enabled=dt16 is not None):
        out = net(a)
    out.backward(up.to(out.dtype))
    res = {"out": out.detach(), "grad_in": a.grad}
    res.update({f"grad {n}": p.grad for n, p in net.named_parameters()})
    return {k: v.detach().cpu().double() for k, v in res.items()}


class _Heads(torch.nn.Module):
    """The three heads of the backbone on their own: `BaseVAMPIRE2._heads` over the same three layers."""

    def __init__(self, mid, num_classes):
        super().__init__()
        from torch import nn
        self.num_classes = num_classes
        self.density_conv = nn.Conv3d(mid, 1, 3, 1, 1, bias=True)
        self.seg_conv = nn.Conv3d(mid, num_classes, 3, 1, 1, bias=True)
        self.rgb_conv = nn.Sequential(nn.Conv3d(mid, 3, 3, 1, 1, bias=True), nn.Sigmoid())

    def forward(self, base):
        from vampire_amd.backbone import BaseVAMPIRE2
        return torch.cat(BaseVAMPIRE2._heads(self, base), 1)


def _nets(which):
    from vampire_amd import backbone
    torch.manual_seed(3)
    if which == "unet":
        return backbone.Unet3D(16, 16), 16
    net = _Heads(16, 18)
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn_like(p) * 0.1)
    return net, 22


def _module_inputs(cout, X=16):
    """Input and upstream gradient at 1 x 16 x 4 x 8 x X.  At X = 16 the UNet's coarsest level is 1 x 2 x 4, below the
    16-bit kernels' X >= 8: conv4 keeps today's torch expressions there, so the comparisons cover that path too.  The
    routing tests count all twelve layers and take X = 32."""
    g = torch.Generator().manual_seed(8)
    return torch.randn(1, 16, 4, 8, X, generator=g), torch.randn(1, cout, 4, 8, X, generator=g)


def _on_off(monkeypatch, net, x, up, dt16):
    from vampire_amd import backbone
    monkeypatch.setattr(backbone.SWITCHES, "conv3d", True)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d_min_voxels", 0)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(backbone.SWITCHES, "conv3d_epilogue", on)
        res[on] = _unet_run(net, x, up, dt16)
    return res


@gpu
@pytest.mark.parametrize("which", ["unet", "heads"])
@pytest.mark.parametrize("dt16", [None, BF16, FP16], ids=["fp32", "bf16", "fp16"])
def test_module_matches_the_switch_off_path(dev, monkeypatch, which, dt16):
    """Unet3D(16, 16) at 1x16x4x8x16 and the heads at the same volume with the switch on and off against the same
    module in float64 on the CPU: the error of every tensor with the switch on is at most twice the switch-off error
    + 1e-6 of its largest magnitude (the bars of test_unet_matches_the_switch_off_path).  In fp32 the forward is
    bit-equal -- but for the rgb head's sigmoid, which has the sigmoid's bar."""
    net, cout = _nets(which)
    x, up = _module_inputs(cout)
    ref = _unet_run(net.double(), x.double(), up.double(), None)
    net = net.float().to(dev)
    res = _on_off(monkeypatch, net, x.to(dev), up.to(dev), dt16)
    failed = []
    if dt16 is None:
        plain = slice(None) if which == "unet" else slice(0, 19)
        if not torch.equal(res[True]["out"][:, plain], res[False]["out"][:, plain]):
            failed.append("fp32 forward is not bit-equal with the switch on and off")
        if which == "heads":
            e_on = float((res[True]["out"][:, 19:] - ref["out"][:, 19:]).abs().max())
            e_off = float((res[False]["out"][:, 19:] - ref["out"][:, 19:]).abs().max())
            if not e_on <= max(2 * e_off, SIG_FLOOR):
                failed.append(f"rgb sigmoid: {e_on:.3e} > max(2 x {e_off:.3e}, 2^-22)")
    assert set(res[True]) == set(ref)
    for k, r in ref.items():
        e_on, e_off = float((res[True][k] - r).abs().max()), float((res[False][k] - r).abs().max())
        lim = 2 * e_off + 1e-6 * float(r.abs().max())
        print(f"[{which}-{DT_NAME[dt16 or F32]}] {k}: err on {e_on:.3e}, off {e_off:.3e}, max |ref| {float(r.abs().max()):.3e}, lim {lim:.3e}")
        if not e_on <= lim:
            failed.append(f"{k}: {e_on:.3e} > {lim:.3e}")
    assert not failed, "; ".join(failed)


def _graph_nodes(tensor):
    seen, stack = set(), [tensor.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        stack.extend(f for f, _ in fn.next_functions)
    return sorted({type(fn).__name__ for fn in seen})


@gpu
def test_no_glue_nodes_behind_the_outputs(dev, monkeypatch):
    """With the switch on (under a bf16 autocast, where all twelve layers have a kernel) the autograd graph behind the
    UNet's output holds no LeakyRelu / Add node, the graph behind the heads' outputs no Slice / Sigmoid node; with it
    off they are there."""
    from vampire_amd import backbone
    monkeypatch.setattr(backbone.SWITCHES, "conv3d", True)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d_min_voxels", 0)
    for which, banned in (("unet", ("LeakyRelu", "AddBackward")), ("heads", ("Slice", "Sigmoid"))):
        net, cout = _nets(which)
        net = net.to(dev)
        x = _module_inputs(cout, 32)[0].to(dev).requires_grad_(True)
        for on in (False, True):
            monkeypatch.setattr(backbone.SWITCHES, "conv3d_epilogue", on)
            with torch.autocast("cuda", dtype=BF16):
                names = _graph_nodes(net(x))
            hits = [n for n in names if any(b in n for b in banned)]
            assert bool(hits) == (not on), (which, on, names)


@gpu
def test_unet_and_heads_routing(dev, monkeypatch):
    """One Unet3D forward + backward under a 16-bit autocast: 12 epilogue forwards (8 stride-1, 4 stride-2) + 1 plain
    one (init_dres) with the switch on, no epilogue entry point with it off; in fp32 the 8 stride-1 layers.  The two
    conv6 have a residual and nothing else: their backward pass is skipped (10 of 12, 6 of 8).  The heads: one epilogue
    forward and one epilogue backward."""
    from vampire_amd import backbone
    log = _record(monkeypatch)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d", True)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d_min_voxels", 0)
    net, _ = _nets("unet")
    net = net.to(dev)
    x, up = (t.to(dev) for t in _module_inputs(16, 32))

    def counts(on, dt16, module=net, grad=up):
        log.clear()
        monkeypatch.setattr(backbone.SWITCHES, "conv3d_epilogue", on)
        _unet_run(module, x, grad, dt16)
        return {n.replace("vamp_conv3d_", ""): log.count(n) for n in sorted(set(log))}

    for dt16 in (BF16, FP16):
        assert counts(True, dt16) == {
            "half_epilogue_forward": 8, "half_s2_epilogue_forward": 4, "half_forward": 1, "epilogue_backward": 10,
            "half_backward_data": 9, "half_backward_weight": 9, "half_s2_backward_data": 4, "half_s2_backward_weight": 4}
        off = counts(False, dt16)
        assert not [n for n in off if "epilogue" in n] and off["half_forward"] == 9 and off["half_s2_forward"] == 4
    assert counts(True, None) == {"epilogue_forward": 8, "forward": 1, "epilogue_backward": 6, "backward_data": 9,
                                  "backward_weight": 9}
    assert not [n for n in counts(False, None) if "epilogue" in n]
    heads, cout = _nets("heads")
    heads = heads.to(dev)
    gup = _module_inputs(cout, 32)[1].to(dev)
    assert counts(True, BF16, heads, gup) == {"half_epilogue_forward": 1, "epilogue_backward": 1, "half_backward_data": 1,
                                              "half_backward_weight": 1}
    assert counts(True, None, heads, gup) == {"epilogue_forward": 1, "epilogue_backward": 1, "backward_data": 1,
                                              "backward_weight": 1}
    assert not [n for n in counts(False, BF16, heads, gup) if "epilogue" in n]


@gpu
def test_biased_layer_reaches_the_kernel_only_with_the_switch(dev, monkeypatch):
    """A `_Conv3` layer built with a bias (BaseLSS / BaseBiLinear's base_conv, feature_conv): MIOpen with the switch
    off, the bias epilogue with it on, the same values either way; parameter names as nn.Conv3d's."""
    from vampire_amd import backbone
    log = _record(monkeypatch)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d", True)
    monkeypatch.setattr(backbone.SWITCHES, "conv3d_min_voxels", 0)
    torch.manual_seed(4)
    layer = backbone._Conv3(16, 16, 3, 1, 1, bias=True).to(dev)
    assert sorted(n for n, _ in layer.named_parameters()) == ["bias", "weight"]
    x = _module_inputs(16)[0].to(dev)
    outs = {}
    for on in (False, True):
        log.clear()
        monkeypatch.setattr(backbone.SWITCHES, "conv3d_epilogue", on)
        a = x.clone().requires_grad_(True)
        y = layer(a)
        y.sum().backward()
        outs[on] = (y.detach(), a.grad, layer.bias.grad.clone())
        layer.zero_grad(set_to_none=True)
        assert ("vamp_conv3d_epilogue_forward" in log) == on and (len(log) > 0) == on, log
    ref = F.conv3d(x.double().cpu(), layer.weight.detach().double().cpu(), layer.bias.detach().double().cpu(), padding=1)
    for on in (False, True):
        close(outs[on][0], ref.float(), what=f"out (switch {on})", atol=1e-5, rtol=1e-5)
    close(outs[True][1], outs[False][1], what="grad_in", atol=1e-5, rtol=1e-5)
    assert bool((outs[True][2].double().cpu() - x.numel() / 16).abs().max() <= 2.0 ** -24 * x.numel() / 16)
