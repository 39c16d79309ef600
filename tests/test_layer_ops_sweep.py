"""The layer operators beside the hot path across the sizes that pick their code paths -- the fp32 and 16-bit 3x3x3
convolutions, the trilinear resize and the voxel pooling of vampire_amd/layers.py, and the glue of ops.py (depth softmax,
density gate, gate + 1x1 conv) -- against float64 CPU references of the same operations (F.conv3d, F.interpolate with
align_corners=True, F.conv2d of the gated tensor, oracle/voxel_pooling_oracle.py, oracle/aten_oracle.py on .double()
inputs): every output and every gradient of every case, from seeded CPU generators.

The case tables hold the smallest shapes that reach a path: each staging depth of the fp32 weight gradient, its chunk
plans and reduce grids, every wave-tile width of the forward with both store kinds; every instantiation of the gate
conv and its degenerate heights; the pooling's lane layouts, list lengths around its two-in-flight loop and cell counts
around the scan tile; the resize's two backward kernels up to the table's capacity (and the refusal beyond it); the
softmax's register / streaming boundary and wave chunks that are all -inf.  The bars are those of the operators' tests
in tests/test_hip_parity.py, quoted below.  The CPU tests at the end map the cases through Python mirrors of the
launchers' host-side dispatch and fail with the name of any branch, instantiation or regime that no case reaches,
compare the mirrors with the library's own host answers (supported / workspace bytes) over grids of descriptors that
include sizes no GPU test could allocate, emulate the resize's table kernel in float32, and pin the wrappers' pointer
alignment guard."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import aten_oracle as O
from oracle import voxel_pooling_oracle as VO
from vampire_amd import _capi
from vampire_amd._tensors import _aligned, _needs_aligned_copy
from vampire_amd.config import CFG_TINY
from test_hip_parity import close, dev, hot  # noqa: F401  (dev: the module-scoped device fixture)

F64 = torch.float64
f32 = np.float32
BF16, FP16 = torch.bfloat16, torch.float16
DT_NAME = {torch.float32: "f32", BF16: "bf16", FP16: "fp16"}

# ------------------------------------------------------------------------------------- the bars (tests/test_hip_parity.py)
# test_conv3d_matches_torch
CONV_OUT = dict(atol=1e-5, rtol=1e-5, scale="max")
CONV_GIN = dict(atol=1e-5, rtol=1e-5, scale="max")
CONV_GW = dict(atol=1e-5, rtol=2e-5, scale="max")
# test_conv3d_bf16_matches_torch (one 16-bit rounding of the output on top of fp32 accumulation)
CONV16_OUT = dict(atol=1e-3, rtol=2.0 ** -8)
CONV16_GIN = dict(atol=1e-3, rtol=2.0 ** -8)
CONV16_GW = dict(atol=1e-6, rtol=2.0 ** -7, scale="max")
# test_gate_conv1x1
GATE_OUT = dict(atol=1e-5, rtol=1e-5, scale="max")
GATE_GRAD = dict(atol=1e-6, rtol=2e-5, scale="max")
# test_resize_full_size (fp32) and test_resize_16bit
RESIZE_OUT = dict(atol=1e-6, rtol=1e-6)
RESIZE_GRAD = dict(atol=1e-5, rtol=1e-5)
RESIZE_ADJOINT = 1e-5                       # |<g, R x> - <R^T g, x>| <= 1e-5 max(1, |<g, R x>|)
RESIZE16_REL = {BF16: 2.0 ** -8, FP16: 2.0 ** -10}
RESIZE16_OUT = lambda dt: dict(atol=1e-3, rtol=RESIZE16_REL[dt])            # noqa: E731
RESIZE16_GRAD = lambda dt: dict(atol=1e-2, rtol=4 * RESIZE16_REL[dt])       # noqa: E731
# test_voxel_pooling_against_numpy_definition (the backward is bit-exact: torch.equal)
POOL_OUT = dict(atol=1e-5, rtol=1e-5, scale="max")
# test_depth_softmax_shapes
SOFTMAX_OUT = dict(atol=1e-6, rtol=1e-5)
SOFTMAX_GRAD = {torch.float32: dict(atol=1e-6, rtol=1e-5, scale="max"), BF16: dict(atol=1e-3, rtol=1e-2, scale="max")}
# test_density_gate_full_size
DGATE_OUT = dict(atol=1e-6, rtol=1e-5)
DGATE_GVO = dict(atol=1e-6, rtol=1e-5)
DGATE_GVD = dict(atol=1e-5, rtol=1e-5, scale="max")

# A case whose fp32 arithmetic alone exceeds its operator's bar gets max(bar, 4 x the error of fp32 aten on the CPU
# against the float64 reference on the same inputs) as its atol, the measured error written next to it; nothing here
# is derived from a kernel's output.  {(test, case, what): (measured fp32-aten error, atol)}
MEASURED = {}


class Compare:
    """Every comparison of a case through test_hip_parity.close, each figure printed before anything asserts; the
    failures of the whole case are raised together at the end."""

    def __init__(self, test, case):
        self.test, self.case, self.failed = test, case, []

    def __call__(self, got, ref, bar, what):
        bar = dict(bar)
        if (self.test, self.case, what) in MEASURED:
            bar["atol"] = max(bar["atol"], MEASURED[(self.test, self.case, what)][1])
        assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
        g, r = got.detach().cpu().double(), ref.detach().cpu().double()
        err = float((g - r).abs().max()) if g.numel() else 0.0
        print(f"[{self.test}:{self.case}] {what}: max err {err:.3e}, max |ref| {float(r.abs().max()) if r.numel() else 0:.3e}, "
              f"bar {bar}")
        assert bool(torch.isfinite(g).all()), f"{what}: non-finite values"
        try:
            close(got, ref.float(), what=what, **bar)
        except AssertionError as e:
            self.failed.append(str(e))

    def equal(self, got, ref, what):
        ok = torch.equal(got.detach().cpu(), ref.detach().cpu())
        print(f"[{self.test}:{self.case}] {what}: bit-exact {ok}")
        if not ok:
            self.failed.append(f"{what}: not bit-exact")

    def done(self):
        assert not self.failed, f"{self.test}[{self.case}]: " + "; ".join(self.failed)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def offset_view(t, dev):
    """t's values in device memory that starts one element past an allocation's first byte: contiguous, but not on a
    16-byte boundary (what a slice of a larger buffer hands a wrapper)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


# =====================================================================================================================
# mirrors of the host-side dispatch
# =====================================================================================================================
def cdiv(a, b):
    return -(-a // b)


def align_up(v, a):
    return cdiv(v, a) * a


I31 = 0x7fffffff

# ------------------------------------------------------------------------------------------------ fp32 conv (conv3d.hip)
WGRAD_THREADS, WGRAD_PRE = 512, 24
CONV_CH = (16, 32)


def conv_check(B, cin, cout, Z, Y, X):
    return (min(B, Z, Y, X) > 0 and cin in CONV_CH and cout in CONV_CH and B * max(cin, cout) * Z * Y * X < I31 * 4)


def conv_npre(cin, cout, X):
    n = cdiv((cin + cout) * X, WGRAD_THREADS)
    return 13 if n <= 13 else (19 if n <= 19 else WGRAD_PRE)


def wgrad_xs(X):
    need = cdiv(X, 4) * 4 + 4
    return cdiv(need - 4, 32) * 32 + 4


def wgrad_lds(cin, cout, X):
    return max((cout + 3 * cin) * wgrad_xs(X), 4 * 9 * 256) * 4


def conv_supported(B, cin, cout, Z, Y, X):
    return int(conv_check(B, cin, cout, Z, Y, X) and (cin + cout) * X <= WGRAD_PRE * WGRAD_THREADS
               and wgrad_lds(cin, cout, X) <= 160 * 1024)


@dataclasses.dataclass(frozen=True)
class WgradPlan:
    per_cu: int
    nchunks: int
    rows_per_chunk: int
    last_rows: int
    nitems: int
    reduce_y: int


def wgrad_plan(B, cin, cout, Z, Y, X):
    combos = B * Z * 3
    lds = wgrad_lds(cin, cout, X)
    per_cu = 3 if lds <= 53 * 1024 else (2 if lds <= 80 * 1024 else 1)
    nchunks = max(1, min(Y, 256 * per_cu // combos))
    rows = cdiv(Y, nchunks)
    nchunks = cdiv(Y, rows)
    nitems = combos * nchunks
    return WgradPlan(per_cu, nchunks, rows, Y - (nchunks - 1) * rows, nitems, max(1, min(16, nitems // 3 // 8)))


def conv_workspace(B, cin, cout, Z, Y, X):
    if not conv_check(B, cin, cout, Z, Y, X):
        return 0
    return align_up(wgrad_plan(B, cin, cout, Z, Y, X).nitems * 9 * cout * cin * 4, 256)


def conv_fwd_plan(B, Z, Y, X):
    """(nm of the wave tiles of a row, waves per workgroup, vector store) of the forward / data-gradient launch."""
    T = cdiv(X, 16)
    tiles_x = cdiv(T, 4)
    base, rem = divmod(T, tiles_x)
    nms = tuple(base + (1 if tx < rem else 0) for tx in range(tiles_x))
    return nms, (8 if B * Z * Y * tiles_x >= 1024 else 4), X % 4 == 0


# --------------------------------------------------------------------------------------- 16-bit conv (conv3d_bf16.hip)
C16_TY, C16_TX, C16_HX, C16_WGS = 4, 64, 68, 512


def tile_ch(c):
    return 16 if c <= 16 else 32


def conv16_supported(B, cin, cout, Z, Y, X):
    return int(1 <= cin <= 32 and 1 <= cout <= 32 and B > 0 and Z > 0 and Y > 0 and X >= 8 and X % 4 == 0
               and Z * Y * X * 32 * 2 < I31)


def conv16_workspace(B, cin, cout, Z, Y, X):
    return C16_WGS * 27 * tile_ch(cin) * tile_ch(cout) * 4 if conv16_supported(B, cin, cout, Z, Y, X) else 0


def conv16_lds(tin, tout):
    return (14 if tin == 16 else 27) * tout * 64 + 3 * (C16_TY + 2) * C16_HX * (tin * 2 + 16)


def conv16_plan(B, cin, cout, Z, Y, X):
    tiles_x = cdiv(X, C16_TX)
    tiles = B * Z * cdiv(Y, C16_TY) * tiles_x
    tin, tout = tile_ch(cin), tile_ch(cout)
    grid = lambda a, b: 256 * (2 if conv16_lds(a, b) <= 78 * 1024 else 1)     # noqa: E731
    return dict(tile=(tin, tout), x8=X % 8 == 0, nnt=tuple(min(4, cdiv(X - tx * C16_TX, 16)) for tx in range(tiles_x)),
                rows=B * Z * Y, tiles=tiles, grid_fwd=grid(tin, tout), grid_dgrad=grid(tout, tin))


# ---------------------------------------------------------------------------------------------- gate conv (gate_conv.hip)
GC_TS, GC_MAX_WGS, GC_LDS_LIMIT = 84, 256, 160 * 1024


def bank_stride(n):
    r = cdiv(n, 16) * 16
    return r if r % 64 in (16, 48) else r + 16


def gc_bwd_lds(mb, nb, oZ):
    cp, kp = mb * 16, nb * 16
    return (cp * bank_stride(kp) + cp * GC_TS + kp * GC_TS + oZ * 64 + 4 * oZ * 64 + kp + cp) * 4


def gc_shape(C_, oZ, cout):
    cin = C_ * oZ
    if cin <= 0 or cout <= 0 or oZ <= 0 or oZ > 32:
        return None
    mb = 1 if cout <= 16 else (5 if cout <= 80 else 0)
    nb = 4 if cin <= 64 else (10 if cin <= 160 else 0)
    if not mb or not nb or gc_bwd_lds(mb, nb, oZ) > GC_LDS_LIMIT:
        return None
    return mb, nb


def gc_workspace(C_, oZ, cout):
    s = gc_shape(C_, oZ, cout)
    return 0 if s is None else (GC_MAX_WGS * s[0] * 16 * s[1] * 16 + GC_MAX_WGS * s[0] * 16) * 4


# ----------------------------------------------------------------------------------------------------- resize (upsample.hip)
MAX_HITS, PLANES_PER_BLOCK = 14, 8


def run_fits(n_in, n_out, hits=MAX_HITS):
    return n_out <= hits if n_in == 1 else 2 * (n_out - 1) // (n_in - 1) + 2 <= hits


def resize_mh(in3, out3):
    """6 / 14: the backward kernel the launcher picks; None: refused."""
    for mh in (6, MAX_HITS):
        if all(run_fits(i, o, mh) for i, o in zip(in3, out3)):
            return mh
    return None


def resize_supported(in3, out3):
    return int(min(in3) > 0 and min(out3) > 0 and resize_mh(in3, out3) is not None)


def resize_workspace(in3):
    return align_up(sum(in3) * 64, 256) if min(in3) > 0 else 0


# ----------------------------------------------------------------------------------------------- pooling (voxel_pooling.hip)
SCAN_TILE, SCAN_PAD = 2048, 64


def pool_plan(C_):
    """(VEC, Q lanes per row, R rows side by side, passes of the scalar path)"""
    vec = C_ % 4 == 0 and C_ <= 256
    return (True, C_ // 4, 64 // (C_ // 4), 0) if vec else (False, 0, 4, cdiv(C_, 64))


def pool_workspace(B, C_, P, nx, ny, nz, code):
    if not (B > 0 and P > 0 and C_ > 0 and nx > 0 and ny > 0 and nz > 0 and B * P < I31 and P < I31
            and B * ny * nx < I31 - 2 * SCAN_TILE and code in (_capi.VAMP_F32, _capi.VAMP_BF16)):
        return 0
    ncell = align_up(B * ny * nx + 1, SCAN_TILE)
    nt = ncell // SCAN_TILE
    return sum(align_up(n, 256) for n in ((ncell + SCAN_PAD) * 4, ncell * 4, nt * 4, nt * 4, (nt + 4) * 4,
                                          B * P * 4, B * P * 4))


# ---------------------------------------------------------------------------------------------- softmax (depth_softmax.hpp)
SM_PIX, SM_SPLIT, SM_REG_BINS = 64, 4, 32


def softmax_reg(D):
    return D <= SM_SPLIT * SM_REG_BINS


def softmax_chunk(D, wave):
    L = cdiv(D, SM_SPLIT)
    return wave * L, min(D, wave * L + L)


# =====================================================================================================================
# the case tables
# =====================================================================================================================
# ---- fp32 conv: name -> (cin, cout, (Z, Y, X), B, grads)
def _cc(cin, cout, vol, B, grads="xw"):
    return (cin, cout, vol, B, grads)


CONV_CASES = {
    "npre19-32to16-x200": _cc(32, 16, (2, 3, 200), 1),
    "npre19-32to32-x108": _cc(32, 32, (2, 3, 108), 1),
    "limit-32to32-x192": _cc(32, 32, (1, 2, 192), 1),
    "limit-16to16-x384": _cc(16, 16, (1, 2, 384), 1),
    "chunk2-last1": _cc(16, 16, (16, 11, 12), 2),
    "nchunks1-z257": _cc(16, 16, (257, 2, 4), 1),
    "one-voxel": _cc(16, 16, (1, 1, 1), 1),
    "x1": _cc(32, 16, (3, 4, 1), 1),
    "x3": _cc(16, 16, (2, 2, 3), 1),
    "y1-16to32": _cc(16, 32, (3, 1, 33), 1),
    "z1-b2": _cc(16, 16, (1, 5, 20), 2),
    "b3-32to32": _cc(32, 32, (2, 3, 20), 3),
    "wpb8-1024-rows": _cc(16, 16, (32, 32, 4), 1),
    "only-weight-grad": _cc(16, 32, (2, 3, 18), 2, "w"),
    "only-input-grad": _cc(32, 16, (2, 3, 18), 2, "x"),
}
CONV_X = (15, 16, 17, 32, 33, 48, 49, 64, 65, 81, 113, 129)
CONV_CASES.update({f"x{X}": _cc(16, 16, (2, 2, X), 1) for X in CONV_X})

# ---- 16-bit conv: name -> (cin, cout, (Z, Y, X), B)
CONV16_CASES = {
    "x8-one-row": (16, 16, (1, 1, 8), 1),
    "y1-x12": (16, 16, (3, 1, 12), 1),
    "x36": (16, 16, (2, 5, 36), 1),
    "x28": (16, 16, (2, 2, 28), 1),
    "x60-16to32": (16, 32, (2, 3, 60), 1),
    "x68-32to16": (32, 16, (2, 2, 68), 1),
    "x16-32to32-b2": (32, 32, (2, 3, 16), 2),
    "ch1to1": (1, 1, (2, 3, 16), 1),
    "ch32to1": (32, 1, (2, 3, 16), 1),
    "ch1to32": (1, 32, (2, 3, 16), 1),
    "ch17to9": (17, 9, (2, 3, 16), 1),
    "ch8to24": (8, 24, (2, 3, 16), 1),
    "rows533": (16, 16, (13, 41, 8), 1),
    "tiles528": (16, 16, (33, 64, 8), 1),
}
CONV16_REFUSED = {"x6": (16, 16, (2, 3, 6), 1), "x10": (16, 16, (2, 3, 10), 1), "cin33": (33, 16, (2, 3, 16), 1)}

# ---- gate conv: name -> (B, C, oZ, oY, oX, Cout, flags)
def _gc(B, C_, oZ, oY, oX, cout, flags=""):
    return (B, C_, oZ, oY, oX, cout, flags)


GATE_CASES = {
    "inst-1x10": _gc(2, 13, 5, 3, 7, 16),
    "inst-5x4": _gc(2, 8, 8, 5, 5, 17),
    "inst-5x10-oZ20": _gc(1, 8, 20, 4, 5, 80),
    "inst-1x4-cin64": _gc(1, 16, 4, 2, 2, 16),
    "no-bias": _gc(2, 5, 6, 3, 11, 24, "nobias"),
    "frozen-weight": _gc(2, 5, 6, 3, 11, 24, "frozen"),
}
GATE_CASES.update({f"oZ{z}": _gc(2, 4, z, 3, 7, 8) for z in (1, 3, 4, 5)})
GATE_CASES.update({f"cells{n}": _gc(3, 4, 3, 1, n, 8) for n in (1, 15, 16, 17, 63, 64, 65)})
GATE_CASES.update({f"cout{n}": _gc(2, 4, 3, 3, 5, n) for n in (1, 16, 17, 80)})

# ---- resize: name -> (B, C, in, out)
RESIZE_CASES = {
    "identity": (1, 3, (4, 5, 6), (4, 5, 6)),
    "to-one-voxel": (1, 2, (3, 4, 5), (1, 1, 1)),
    "to-one-plane": (1, 2, (3, 4, 5), (1, 9, 5)),
    "from-one-voxel-14": (1, 1, (1, 1, 1), (14, 14, 14)),
    "capacity-7-6-7": (2, 4, (2, 3, 3), (7, 6, 7)),
    "down-ragged-9planes": (1, 9, (9, 7, 11), (4, 3, 5)),
    "mixed-up-down-same": (1, 8, (5, 6, 7), (9, 3, 7)),
    "mh6-limit": (1, 2, (3, 4, 2), (5, 7, 3)),
}
RESIZE_REFUSED = (1, 1, (2, 2, 2), (8, 8, 8))        # 2 * 7 / 1 + 2 = 16 > 14
RESIZE_DTYPES = (torch.float32, BF16, FP16)

# ---- pooling
POOL_CHANNELS = (1, 4, 12, 64, 128, 256, 260, 70)
POOL_DTYPES = (torch.float32, BF16)
# cells B * ny * nx around the 2048-cell scan tile: name -> (B, (nx, ny))
POOL_GRIDS = {"cells2047": (1, (23, 89)), "cells2048": (2, (32, 32)), "cells2049": (1, (3, 683)), "cells4096": (4, (32, 32))}
POOL_LIST_MULTIPLES = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1), (5, 2))       # a R + b points in a cell

# ---- softmax / density gate
SOFTMAX_D = (1, 4, 5, 127, 128, 129, 200)
SOFTMAX_HW = (1, 63, 64, 65)
SOFTMAX_DTYPES = (torch.float32, BF16)
# -inf chunks: name -> (D, dtype, first bin, last bin + 1 of the -inf run (for the pixels chosen), single finite bin)
SOFTMAX_INF = {
    "reg-chunk1": (8, torch.float32, 2, 4, None),
    "reg-chunk0-bf16": (8, BF16, 0, 2, None),
    "stream-chunk2": (200, torch.float32, 100, 150, None),
    "stream-chunk0-bf16": (200, BF16, 0, 50, None),
    "reg-single-finite": (8, torch.float32, 0, 8, 5),
    "stream-single-finite": (200, torch.float32, 0, 200, 199),
}
DGATE_C = (1, 5)
DGATE_CELLS = (1, 255, 256, 257)


# =====================================================================================================================
# GPU comparisons
# =====================================================================================================================
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------- fp32 conv
def _conv_inputs(cin, cout, vol, B, seed, dt=torch.float32):
    g = gen(seed)
    x = torch.randn(B, cin, *vol, generator=g).to(dt)
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.05).to(dt)
    up = torch.randn(B, cout, *vol, generator=g).to(dt)
    return x, w, up


def _conv_reference(x, w, up):
    a, wa = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = F.conv3d(a, wa, padding=1)
    ref.backward(up.double())
    return ref.detach(), a.grad, wa.grad


def _run_conv(cmp, fn, x, w, up, grads, bars, dev, put=lambda t, dev: t.to(dev)):
    ref, gx, gw = _conv_reference(x, w, up)
    b = put(x, dev).requires_grad_("x" in grads)
    wb = put(w, dev).requires_grad_("w" in grads)
    out = fn(b, wb)
    assert out.dtype == x.dtype
    cmp(out, ref, bars[0], "out")
    out.backward(put(up, dev))
    if "x" in grads:
        assert b.grad.dtype == x.dtype
        cmp(b.grad, gx, bars[1], "grad_in")
    else:
        assert b.grad is None
    if "w" in grads:
        assert wb.grad.dtype == w.dtype
        cmp(wb.grad, gw, bars[2], "grad_weight")
    else:
        assert wb.grad is None
    cmp.done()


@gpu
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv3d_fp32(dev, name):
    """The fp32 matrix-core conv against F.conv3d in float64: output, data gradient, weight gradient."""
    from vampire_amd.ops import conv3d_3x3x3, conv3d_supported
    cin, cout, vol, B, grads = CONV_CASES[name]
    x, w, up = _conv_inputs(cin, cout, vol, B, 11)
    assert conv3d_supported(x.to(dev), w.to(dev), (1, 1, 1), (1, 1, 1), None)
    _run_conv(Compare("conv3d", name), conv3d_3x3x3, x, w, up, grads, (CONV_OUT, CONV_GIN, CONV_GW), dev)


@gpu
def test_conv3d_fp32_misaligned_views(dev):
    """Input, weight and upstream gradient as views that start 4 bytes past a 16-byte boundary: the wrapper copies
    them (the kernels use 16-byte vector accesses), the results are those of the aligned tensors."""
    from vampire_amd.ops import conv3d_3x3x3
    x, w, up = _conv_inputs(16, 16, (2, 3, 20), 2, 12)
    _run_conv(Compare("conv3d", "misaligned"), conv3d_3x3x3, x, w, up, "xw", (CONV_OUT, CONV_GIN, CONV_GW), dev,
              put=offset_view)


# -------------------------------------------------------------------------------------------------------- 16-bit conv
@gpu
@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", list(CONV16_CASES))
def test_conv3d_16bit(dev, name, dt):
    """The 16-bit matrix-core conv (fp32 accumulation) against F.conv3d in float64 on the same rounded operands."""
    from vampire_amd.ops import conv3d_bf16, conv3d_bf16_supported
    cin, cout, vol, B = CONV16_CASES[name]
    x, w, up = _conv_inputs(cin, cout, vol, B, 4, dt)
    assert conv3d_bf16_supported(x.to(dev), w.to(dev), (1, 1, 1), (1, 1, 1), None)
    _run_conv(Compare("conv3d_16bit", f"{name}-{DT_NAME[dt]}"), conv3d_bf16, x, w, up, "xw",
              (CONV16_OUT, CONV16_GIN, CONV16_GW), dev)


@gpu
@pytest.mark.parametrize("name", list(CONV16_REFUSED))
def test_conv3d_16bit_refuses(dev, name):
    from vampire_amd.ops import conv3d_bf16, conv3d_bf16_supported
    cin, cout, vol, B = CONV16_REFUSED[name]
    x, w, _ = _conv_inputs(cin, cout, vol, B, 4, BF16)
    assert not conv3d_bf16_supported(x.to(dev), w.to(dev), (1, 1, 1), (1, 1, 1), None)
    with pytest.raises(_capi.VampireHipError):
        conv3d_bf16(x.to(dev), w.to(dev))


@gpu
@pytest.mark.parametrize("dt", [BF16, FP16], ids=["bf16", "fp16"])
def test_conv3d_16bit_misaligned_views(dev, dt):
    """Views that start 2 bytes past a 16-byte boundary: the forward stages its input with dword buffer loads and the
    weight gradient with 8- and 16-byte loads; the wrapper's guard copies, the kernels never see the pointer."""
    from vampire_amd.ops import conv3d_bf16
    x, w, up = _conv_inputs(16, 16, (2, 3, 20), 2, 5, dt)
    _run_conv(Compare("conv3d_16bit", f"misaligned-{DT_NAME[dt]}"), conv3d_bf16, x, w, up, "xw",
              (CONV16_OUT, CONV16_GIN, CONV16_GW), dev, put=offset_view)


# ---------------------------------------------------------------------------------------------------------- gate conv
@gpu
@pytest.mark.parametrize("mode", ["sdf", "naive"])
@pytest.mark.parametrize("name", list(GATE_CASES))
def test_gate_conv1x1(dev, name, mode):
    """Gate + 1x1 conv against F.conv2d of the gated tensor in float64: the output and all (up to) four gradients, and
    the same bits on a second run."""
    B, C_, oZ, oY, oX, cout, flags = GATE_CASES[name]
    hp = hot(dataclasses.replace(CFG_TINY, density_mode=mode), dev)
    assert hp.gate_conv1x1_supported(C_, oZ, cout)
    g = gen(5)
    vo, vd = torch.randn(B, C_, oZ, oY, oX, generator=g), torch.randn(B, 1, oZ, oY, oX, generator=g)
    w = torch.randn(cout, C_ * oZ, 1, 1, generator=g) * 0.1
    bs = None if flags == "nobias" else torch.randn(cout, generator=g)
    go = torch.randn(B, cout, oY, oX, generator=g)
    names = ["voxel_output", "voxel_density", "weight", "bias"]
    wants = [True, True, flags != "frozen", True]

    def leaves(to):
        return [None if t is None else to(t).requires_grad_(k) for t, k in zip((vo, vd, w, bs), wants)]
    ra = leaves(lambda t: t.double())
    gate = ra[1].tanh() if mode == "sdf" else ra[1]
    ref = F.conv2d((ra[0] * gate).reshape(B, C_ * oZ, oY, oX), ra[2], ra[3])
    ref.backward(go.double())
    cmp = Compare("gate_conv1x1", f"{name}-{mode}")
    la = leaves(lambda t: t.to(dev))
    out = hp.gate_conv1x1(*la)
    cmp(out, ref.detach(), GATE_OUT, "out")
    out.backward(go.to(dev))
    lb = leaves(lambda t: t.to(dev))
    hp.gate_conv1x1(*lb).backward(go.to(dev))
    for a, b_, r, n, k in zip(la, lb, ra, names, wants):
        if a is None:
            continue
        if not k:
            assert a.grad is None
            continue
        cmp(a.grad, r.grad, GATE_GRAD, "grad " + n)
        cmp.equal(b_.grad, a.grad, "second run grad " + n)
    cmp.done()


# ------------------------------------------------------------------------------------------------------------- resize
def _resize_inputs(B, C_, in3, out3, dt):
    g = gen(9)
    x = torch.randn(B, C_, *in3, generator=g).to(dt)
    up = torch.randn(B, C_, *out3, generator=g).to(dt)
    return x, up


def _run_resize(cmp, x, up, out3, dt, dev, put=lambda t, dev: t.to(dev)):
    from vampire_amd.ops import upsample_trilinear
    a = x.double().requires_grad_(True)
    ref = F.interpolate(a, out3, mode="trilinear", align_corners=True)
    ref.backward(up.double())
    b = put(x, dev).requires_grad_(True)
    got = upsample_trilinear(b, out3)
    assert got.dtype == dt and got.shape == ref.shape
    got.backward(put(up, dev))
    assert b.grad.dtype == dt
    if dt == torch.float32:
        cmp(got, ref.detach(), RESIZE_OUT, "out")
        cmp(b.grad, a.grad, RESIZE_GRAD, "grad")
    else:
        cmp(got, ref.detach(), RESIZE16_OUT(dt), "out")
        cmp(b.grad, a.grad, RESIZE16_GRAD(dt), "grad")
    # the adjoint identity <g, R x> == <R^T g, x>, both sides summed in float64 from the kernels' results
    l_terms = up.double() * got.detach().cpu().double()
    r_terms = b.grad.cpu().double() * x.double()
    lhs, rhs = float(l_terms.sum()), float(r_terms.sum())
    lim = RESIZE_ADJOINT * max(1.0, abs(lhs))
    if dt != torch.float32:
        # every element of R x and of R^T g carries one rounding to dt, relative error <= half an ulp: the two sums
        # may move by that fraction of their terms' magnitudes (2^-9 for bf16, 2^-11 for fp16), nothing else is added
        half_ulp = 2.0 ** -9 if dt == BF16 else 2.0 ** -11
        lim += half_ulp * (float(l_terms.abs().sum()) + float(r_terms.abs().sum()))
    print(f"[resize:{cmp.case}] adjoint: <g, R x> {lhs:.9e}, <R^T g, x> {rhs:.9e}, |diff| {abs(lhs - rhs):.3e}, lim {lim:.3e}")
    if not abs(lhs - rhs) <= lim:
        cmp.failed.append(f"adjoint identity: {lhs} vs {rhs} (lim {lim})")
    cmp.done()


@gpu
@pytest.mark.parametrize("dt", RESIZE_DTYPES, ids=[DT_NAME[d] for d in RESIZE_DTYPES])
@pytest.mark.parametrize("name", list(RESIZE_CASES))
def test_resize(dev, name, dt):
    """The trilinear resize against F.interpolate(align_corners=True) in float64 (on the rounded values for the 16-bit
    types): forward, the table-gather backward on the kernel the sizes pick, and the adjoint identity."""
    B, C_, in3, out3 = RESIZE_CASES[name]
    assert _capi.load().vamp_upsample_trilinear_supported(*in3, *out3) == 1
    x, up = _resize_inputs(B, C_, in3, out3, dt)
    _run_resize(Compare("resize", f"{name}-{DT_NAME[dt]}"), x, up, out3, dt, dev)


@gpu
@pytest.mark.parametrize("dt", [torch.float32, BF16], ids=["f32", "bf16"])
def test_resize_misaligned_views(dev, dt):
    B, C_, in3, out3 = RESIZE_CASES["mixed-up-down-same"]
    x, up = _resize_inputs(B, C_, in3, out3, dt)
    _run_resize(Compare("resize", f"misaligned-{DT_NAME[dt]}"), x, up, out3, dt, dev, put=offset_view)


@gpu
def test_resize_refuses_a_ratio_beyond_the_table(dev):
    """2 -> 8 would need 16 table slots per source index: the library says so, the backward raises instead of dropping
    the hits beyond the 14th, and the library works afterwards."""
    from vampire_amd.ops import upsample_trilinear
    B, C_, in3, out3 = RESIZE_REFUSED
    lib = _capi.load()
    assert lib.vamp_upsample_trilinear_supported(*in3, *out3) == 0
    x, up = _resize_inputs(B, C_, in3, out3, torch.float32)
    b = x.to(dev).requires_grad_(True)
    got = upsample_trilinear(b, out3)
    close(got, F.interpolate(x.double(), out3, mode="trilinear", align_corners=True).float(), what="forward", **RESIZE_OUT)
    with pytest.raises(_capi.VampireHipError):
        got.backward(up.to(dev))
    B, C_, in3, out3 = RESIZE_CASES["identity"]
    x, up = _resize_inputs(B, C_, in3, out3, torch.float32)
    _run_resize(Compare("resize", "after-refusal"), x, up, out3, torch.float32, dev)


# ------------------------------------------------------------------------------------------------------------ pooling
def _run_pool(cmp, geom, feat, vn, dev, put=lambda t, dev: t.to(dev)):
    """geom [B, P, 3] (int32 | int64), feat [B, P, C] (fp32 | bf16) in the operator's six-dimensional layout."""
    from vampire_amd.ops import voxel_pooling
    B, P, C_ = feat.shape
    dt = feat.dtype
    f_d = put(feat.reshape(B, 1, 1, 1, P, C_), dev).requires_grad_(True)
    out = voxel_pooling(put(geom.reshape(B, 1, 1, 1, P, 3), dev), f_d, vn)
    assert out.shape == (B, C_, vn[1], vn[0]) and out.dtype == torch.float32
    want = VO.voxel_pooling(geom.numpy(), feat.float().numpy(), vn)
    cmp(out, torch.from_numpy(want), POOL_OUT, "out")
    go = torch.randn(out.shape, generator=gen(13))
    out.backward(put(go, dev))
    gw = VO.voxel_pooling_backward(geom.numpy(), go.numpy(), vn)
    assert f_d.grad.dtype == dt
    cmp.equal(f_d.grad.float().cpu().reshape(B, P, C_), torch.from_numpy(gw).to(dt).float(), "grad_feat")
    cmp.done()


def _random_geom(B, P, vn, g, dtype=torch.int64):
    nx, ny, nz = vn
    return torch.stack([torch.randint(-1, nx + 1, (B, P), generator=g), torch.randint(-1, ny + 1, (B, P), generator=g),
                        torch.randint(-1, nz + 1, (B, P), generator=g)], -1).to(dtype)


def pool_list_geometry(C_):
    """(geom [1, P, 3], voxel_num, points per cell): cell k of a 7 x 1 x 2 grid holds exactly a R + b points for the
    (a, b) of POOL_LIST_MULTIPLES (R rows side by side in the gather, four in the scalar path), at both heights, in a
    shuffled order, among points outside the grid on every side."""
    R = pool_plan(C_)[2]
    counts = [a * R + b for a, b in POOL_LIST_MULTIPLES]
    pts = [(k, 0, i % 2) for k, n in enumerate(counts) for i in range(n)]
    pts += [(-1, 0, 0), (len(counts), 0, 1), (0, -1, 0), (0, 1, 1), (1, 0, -1), (1, 0, 2)] * 3
    geom = torch.tensor(pts, dtype=torch.int64)[torch.randperm(len(pts), generator=gen(3))]
    return geom[None], (len(counts), 1, 2), counts


@gpu
@pytest.mark.parametrize("dt", POOL_DTYPES, ids=[DT_NAME[d] for d in POOL_DTYPES])
@pytest.mark.parametrize("C_", POOL_CHANNELS)
def test_voxel_pooling_channels(dev, C_, dt):
    """Every lane layout of the gather (Q = C / 4 lanes per row, or the scalar passes) over a grid with three heights
    (z drawn from [-1, 4): a point at any in-range height lands in its BEV cell) and int64 indices."""
    g = gen(11)
    vn = (5, 4, 3)
    geom = _random_geom(2, 90, vn, g)
    geom[0, :40] = torch.tensor([2, 3, 1])                       # one crowded cell at z = 1
    assert int(((geom[..., 2] > 0) & (geom[..., 2] < 3)).sum()) > 20
    feat = torch.randn(2, 90, C_, generator=g).to(dt)
    _run_pool(Compare("voxel_pooling", f"C{C_}-{DT_NAME[dt]}"), geom, feat, vn, dev)


@gpu
@pytest.mark.parametrize("dt", POOL_DTYPES, ids=[DT_NAME[d] for d in POOL_DTYPES])
@pytest.mark.parametrize("C_", POOL_CHANNELS)
def test_voxel_pooling_list_lengths(dev, C_, dt):
    """Cells of exactly 0, 1, R, R + 1, 2 R, 2 R + 1 and 5 R + 2 points: every exit of the two-in-flight loop."""
    geom, vn, _ = pool_list_geometry(C_)
    feat = torch.randn(1, geom.shape[1], C_, generator=gen(12)).to(dt)
    _run_pool(Compare("voxel_pooling", f"lists-C{C_}-{DT_NAME[dt]}"), geom.to(torch.int32), feat, vn, dev)


@gpu
@pytest.mark.parametrize("dt", POOL_DTYPES, ids=[DT_NAME[d] for d in POOL_DTYPES])
@pytest.mark.parametrize("name", list(POOL_GRIDS))
def test_voxel_pooling_scan_tile_boundary(dev, name, dt):
    """Cell counts at and around the 2048-cell scan tile: the gather reads a cell's end from the next cell's start,
    which for the last cell of a tile lies in the next tile (or is the grand total behind the last cell)."""
    B, (nx, ny) = POOL_GRIDS[name]
    vn = (nx, ny, 2)
    g = gen(14)
    geom = _random_geom(B, 700, vn, g, torch.int32)
    cells = B * ny * nx
    for k, c in enumerate(sorted({0, SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, 2 * SCAN_TILE - 1, cells - 1})):
        if c < cells:                        # 3 + k points in the cells either side of every tile edge
            b, r = divmod(c, ny * nx)
            geom[b, 10 * k:10 * k + 3 + k] = torch.tensor([r % nx, r // nx, k % 2], dtype=torch.int32)
    feat = torch.randn(B, 700, 8, generator=g).to(dt)
    _run_pool(Compare("voxel_pooling", f"{name}-{DT_NAME[dt]}"), geom, feat, vn, dev)


@gpu
@pytest.mark.parametrize("dt", POOL_DTYPES, ids=[DT_NAME[d] for d in POOL_DTYPES])
@pytest.mark.parametrize("P", [1, 37, 63])
def test_voxel_pooling_few_points(dev, P, dt):
    g = gen(15)
    vn = (3, 2, 2)
    _run_pool(Compare("voxel_pooling", f"P{P}-{DT_NAME[dt]}"), _random_geom(2, P, vn, g, torch.int32),
              torch.randn(2, P, 20, generator=g).to(dt), vn, dev)


@gpu
@pytest.mark.parametrize("dt", POOL_DTYPES, ids=[DT_NAME[d] for d in POOL_DTYPES])
def test_voxel_pooling_misaligned_views(dev, dt):
    """Features, indices and the upstream gradient as views off a 16-byte boundary (the gather reads 8- and 16-byte
    rows): the wrapper copies them."""
    g = gen(16)
    vn = (5, 4, 3)
    _run_pool(Compare("voxel_pooling", f"misaligned-{DT_NAME[dt]}"), _random_geom(2, 90, vn, g, torch.int32),
              torch.randn(2, 90, 12, generator=g).to(dt), vn, dev, put=offset_view)


# ----------------------------------------------------------------------------------------- depth softmax, density gate
def _run_softmax(cmp, lg, up, dev, tag=""):
    dt = lg.dtype
    ref_in = lg.double().requires_grad_(True)
    ref = O.depth_softmax(ref_in)
    assert ref.dtype == F64 and bool(torch.isfinite(ref).all())
    ref.backward(up.double())
    x = lg.to(dev).requires_grad_(True)
    got = hot(CFG_TINY, dev).depth_softmax(x)
    assert got.dtype == torch.float32
    cmp(got, ref.detach(), SOFTMAX_OUT, tag + "softmax")
    got.backward(up.to(dev))
    assert x.grad.dtype == dt
    cmp(x.grad, ref_in.grad, SOFTMAX_GRAD[dt], tag + "grad")


@gpu
@pytest.mark.parametrize("dt", SOFTMAX_DTYPES, ids=[DT_NAME[d] for d in SOFTMAX_DTYPES])
@pytest.mark.parametrize("D", SOFTMAX_D)
def test_depth_softmax(dev, D, dt):
    """Depth counts either side of the register / streaming boundary (and fewer bins than waves) at pixel counts around
    the 64-pixel tile, two images, against the oracle in float64."""
    cmp = Compare("depth_softmax", f"D{D}-{DT_NAME[dt]}")
    for HW in SOFTMAX_HW:
        g = gen(3 + HW)
        lg = (torch.randn(2, D, 1, HW, generator=g) * 4.0).to(dt)
        _run_softmax(cmp, lg, torch.randn(2, D, 1, HW, generator=g), dev, f"HW{HW} ")
    cmp.done()


@gpu
@pytest.mark.parametrize("name", list(SOFTMAX_INF))
def test_depth_softmax_masked_chunks(dev, name):
    """Masked depth bins: for every third pixel the whole depth chunk of one wave is -inf (its local maximum is -inf
    and must drop out of the merge), or all bins but one; the probabilities there are finite, the gradient zero."""
    D, dt, d0, d1, keep = SOFTMAX_INF[name]
    g = gen(7)
    lg = torch.randn(2, D, 1, 70, generator=g) * 4.0
    lg[:, d0:d1, :, ::3] = float("-inf")
    if keep is not None:
        lg[:, keep, :, ::3] = torch.randn(2, 1, 24, generator=g)
    cmp = Compare("depth_softmax", name)
    _run_softmax(cmp, lg.to(dt), torch.randn(2, D, 1, 70, generator=g), dev)
    cmp.done()


@gpu
@pytest.mark.parametrize("mode", ["sdf", "naive"])
@pytest.mark.parametrize("C_", DGATE_C)
def test_density_gate(dev, C_, mode):
    hp = hot(dataclasses.replace(CFG_TINY, density_mode=mode), dev)
    cmp = Compare("density_gate", f"C{C_}-{mode}")
    for cells in DGATE_CELLS:
        g = gen(4 + cells)
        shape = (3, C_, 1, 1, cells)
        vo, vd = torch.randn(shape, generator=g), torch.rand((3, 1, 1, 1, cells), generator=g) * 4.0 - 1.0
        up = torch.randn(shape, generator=g)
        a, b = vo.double().requires_grad_(True), vd.double().requires_grad_(True)
        ref = O.density_gate(a, b, mode)
        ref.backward(up.double())
        x, y = vo.to(dev).requires_grad_(True), vd.to(dev).requires_grad_(True)
        out = hp.density_gate(x, y)
        cmp(out, ref.detach(), DGATE_OUT, f"cells{cells} gated")
        out.backward(up.to(dev))
        cmp(x.grad, a.grad, DGATE_GVO, f"cells{cells} grad_voxel_output")
        cmp(y.grad, b.grad, DGATE_GVD, f"cells{cells} grad_voxel_density")
    cmp.done()


# =====================================================================================================================
# CPU tests: what the cases reach, the mirrors against the library, the resize table, the alignment guard
# =====================================================================================================================
def _unreached(required, reached):
    return sorted(str(r) for r in set(required) - set(reached))


def test_conv3d_fp32_cases_reach_every_path():
    reached = set()
    for name, (cin, cout, (Z, Y, X), B, grads) in CONV_CASES.items():
        assert conv_supported(B, cin, cout, Z, Y, X), name
        pl = wgrad_plan(B, cin, cout, Z, Y, X)
        nms, wpb, vec = conv_fwd_plan(B, Z, Y, X)
        reached |= {f"npre{conv_npre(cin, cout, X)}", f"inst{cin}to{cout}", f"per_cu{pl.per_cu}", f"wpb{wpb}",
                    f"grads-{grads}"}
        if (cin + cout) * X == WGRAD_PRE * WGRAD_THREADS:
            reached.add("staging-limit")
        if pl.rows_per_chunk > 1 and pl.nchunks > 1 and pl.last_rows < pl.rows_per_chunk:
            reached.add("chunk-rows>1-short-last")
        if pl.rows_per_chunk > 1 and pl.nchunks > 1 and pl.last_rows == pl.rows_per_chunk:
            reached.add("chunk-rows>1-even")
        if pl.nchunks == 1 and Y > 1 and B * Z * 3 > 256 * pl.per_cu:
            reached.add("nchunks1-by-combos")
        if pl.rows_per_chunk == 1 and Y > 1:
            reached.add("one-row-chunks")
        reached.add("reduce-y1" if pl.reduce_y == 1 else ("reduce-y16" if pl.reduce_y == 16 else "reduce-y2..15"))
        reached |= {k for k, v in (("Z1", Z == 1), ("Y1", Y == 1), ("X<4", X < 4), ("B>1", B > 1)) if v}
        kind = "vec" if vec else "scalar"
        if len(set(nms)) == 1:
            reached.add(f"nm{nms[0]}-{'alone' if len(nms) == 1 else 'repeated'}-{kind}")
        else:
            reached.add(f"nm-mixed-{kind}")
        reached |= {f"nm{n}-{kind}" for n in nms}
        if X % 16 and X % 4 == 0:
            reached.add("vec-store-ragged-tile")       # X % 4 == 0 with a partly filled last M tile
    required = ({f"npre{n}" for n in (13, 19, 24)} | {f"inst{a}to{b}" for a in CONV_CH for b in CONV_CH}
                | {f"per_cu{n}" for n in (1, 2, 3)} | {"wpb4", "wpb8", "grads-xw", "grads-x", "grads-w", "staging-limit",
                                                       "chunk-rows>1-short-last", "nchunks1-by-combos", "one-row-chunks",
                                                       "reduce-y1", "reduce-y16", "reduce-y2..15", "Z1", "Y1", "X<4", "B>1",
                                                       "nm-mixed-vec", "nm-mixed-scalar", "vec-store-ragged-tile"}
                | {f"nm{n}-alone-{k}" for n in (1, 2, 3, 4) for k in ("vec", "scalar")}
                | {f"nm{n}-{k}" for n in (1, 2, 3, 4) for k in ("vec", "scalar")})
    assert not _unreached(required, reached), f"fp32 conv paths no case reaches: {_unreached(required, reached)}"
    # what the issue's arithmetic says of single cases
    assert conv_npre(32, 16, 200) == 19 and conv_npre(32, 32, 108) == 19
    pl = wgrad_plan(2, 16, 16, 16, 11, 12)
    assert (pl.nchunks, pl.rows_per_chunk, pl.last_rows, pl.reduce_y) == (6, 2, 1, 16)
    assert wgrad_plan(1, 16, 16, 257, 2, 4).nchunks == 1 and wgrad_plan(1, 16, 16, 1, 1, 1).reduce_y == 1


def test_conv3d_16bit_cases_reach_every_path():
    reached = set()
    for name, (cin, cout, (Z, Y, X), B) in CONV16_CASES.items():
        assert conv16_supported(B, cin, cout, Z, Y, X), name
        p = conv16_plan(B, cin, cout, Z, Y, X)
        reached |= {f"tile{p['tile'][0]}x{p['tile'][1]}", "x8" if p["x8"] else "x4", f"grid{p['grid_fwd']}",
                    f"dgrid{p['grid_dgrad']}"}
        reached |= {f"nnt{n}" for n in p["nnt"]}
        if len(p["nnt"]) > 1 and p["nnt"][-1] == 1:
            reached.add("second-x-tile-one-n-tile")
        if p["rows"] > C16_WGS and p["rows"] % C16_WGS:
            reached.add("rows>512-remainder")
        if p["tiles"] > p["grid_fwd"] and p["tiles"] % p["grid_fwd"]:
            reached.add("tiles>grid-remainder")
        reached |= {k for k, v in (("Z1", Z == 1), ("Y1", Y == 1), ("X8", X == 8), ("B>1", B > 1),
                                   ("Y%4", Y % C16_TY != 0)) if v}
        reached |= {f"cin{cin}" for _ in [0] if cin not in (16, 32)} | {f"cout{cout}" for _ in [0] if cout not in (16, 32)}
    required = ({f"tile{a}x{b}" for a in (16, 32) for b in (16, 32)} | {f"nnt{n}" for n in (1, 2, 3, 4)}
                | {"x8", "x4", "grid512", "grid256", "dgrid512", "dgrid256", "second-x-tile-one-n-tile",
                   "rows>512-remainder", "tiles>grid-remainder", "Z1", "Y1", "X8", "B>1", "Y%4",
                   "cin1", "cin8", "cin17", "cout1", "cout9", "cout24"})
    assert not _unreached(required, reached), f"16-bit conv paths no case reaches: {_unreached(required, reached)}"
    for name, (cin, cout, (Z, Y, X), B) in CONV16_REFUSED.items():
        assert not conv16_supported(B, cin, cout, Z, Y, X), name


def test_gate_conv_cases_reach_every_path():
    reached = set()
    for name, (B, C_, oZ, oY, oX, cout, flags) in GATE_CASES.items():
        s = gc_shape(C_, oZ, cout)
        assert s is not None, name
        cells = oY * oX
        reached |= {f"inst{s[0]}x{s[1]}", f"cout{cout}", f"flags-{flags or 'all'}"}
        reached.add("zstep0" if 4 % oZ == 0 else ("zstep1-oZ3" if oZ == 3 else "zstep4"))
        reached |= {f"oZ{oZ}" for _ in [0] if oZ in (1, 3, 4)}
        reached |= {k for k, v in (("cells<16", cells < 16), ("cells%16", cells % 16 != 0), ("cells=16", cells == 16),
                                   ("cells%64", cells % 64 != 0), ("cells=64", cells == 64), ("cells>64", cells > 64),
                                   ("B>1", B > 1), ("cin=64", C_ * oZ == 64)) if v}
        if s == (5, 10) and gc_shape(C_, oZ + 1, cout) is None and oZ < 32:
            reached.add("inst5x10-at-lds-limit")
    required = ({f"inst{m}x{n}" for m in (1, 5) for n in (4, 10)} | {f"cout{n}" for n in (1, 16, 17, 80)}
                | {"flags-all", "flags-nobias", "flags-frozen", "zstep0", "zstep1-oZ3", "zstep4", "oZ1", "oZ3", "oZ4",
                   "cells<16", "cells%16", "cells=16", "cells%64", "cells=64", "cells>64", "B>1", "cin=64",
                   "inst5x10-at-lds-limit"})
    assert not _unreached(required, reached), f"gate conv paths no case reaches: {_unreached(required, reached)}"
    # the rule the refusal message and the header state: the LDS image caps <5,10> at oZ = 20, nothing else below 32
    assert gc_shape(8, 20, 80) == (5, 10) and gc_shape(7, 21, 80) is None and gc_shape(3, 21, 80) == (5, 4)
    assert gc_shape(5, 32, 16) == (1, 10) and gc_shape(2, 32, 80) == (5, 4) and gc_shape(1, 33, 8) is None
    assert gc_bwd_lds(5, 10, 20) <= GC_LDS_LIMIT < gc_bwd_lds(5, 10, 21)


def test_resize_cases_reach_every_path():
    reached = set()
    for name, (B, C_, in3, out3) in RESIZE_CASES.items():
        mh = resize_mh(in3, out3)
        assert mh is not None, name
        reached.add(f"mh{mh}")
        if in3 == out3:
            reached.add("identity")
        for i, o in zip(in3, out3):
            reached |= {k for k, v in (("out1-in>1", o == 1 and i > 1), ("in1-out14", i == 1 and o == MAX_HITS),
                                       ("fits-exactly-14", i > 1 and 2 * (o - 1) // (i - 1) + 2 == MAX_HITS),
                                       ("fits-exactly-6", i > 1 and 2 * (o - 1) // (i - 1) + 2 == 6),
                                       ("fits-7", i > 1 and 2 * (o - 1) // (i - 1) + 2 == 7),
                                       ("down-non-integer", i > o > 1 and (i - 1) % (o - 1) != 0),
                                       ("up-non-integer", 1 < i < o and (o - 1) % (i - 1) != 0)) if v}
        if len({(i > o) - (i < o) for i, o in zip(in3, out3)}) == 3:
            reached.add("up-down-same-mixed")
        planes = B * C_
        reached |= {k for k, v in (("planes=8", planes == PLANES_PER_BLOCK), ("planes=9", planes == PLANES_PER_BLOCK + 1),
                                   ("planes<8", planes < PLANES_PER_BLOCK)) if v}
    required = {"mh6", "mh14", "identity", "out1-in>1", "in1-out14", "fits-exactly-14", "fits-exactly-6", "fits-7",
                "down-non-integer", "up-non-integer", "up-down-same-mixed", "planes=8", "planes=9", "planes<8"}
    assert not _unreached(required, reached), f"resize paths no case reaches: {_unreached(required, reached)}"
    assert resize_mh(*RESIZE_REFUSED[2:]) is None and not resize_supported(*RESIZE_REFUSED[2:])
    assert RESIZE_DTYPES == (torch.float32, BF16, FP16)          # each of them runs every case: both kernels


def test_pooling_cases_reach_every_path():
    reached = set()
    for C_ in POOL_CHANNELS:
        vec, Q, R, passes = pool_plan(C_)
        reached.add(f"Q{Q}" if vec else f"scalar-{'one-pass' if passes == 1 else 'multi-pass'}")
        if not vec and C_ % 4 == 0:
            reached.add("C%4==0-above-256")
        geom, vn, counts = pool_list_geometry(C_)
        assert counts == [a * R + b for a, b in POOL_LIST_MULTIPLES] and vn[2] > 1
        ok = ((geom[0, :, 0] >= 0) & (geom[0, :, 0] < vn[0]) & (geom[0, :, 1] == 0) & (geom[0, :, 2] >= 0) & (geom[0, :, 2] < vn[2]))
        assert torch.bincount(geom[0, ok, 0], minlength=vn[0]).tolist() == counts and int((~ok).sum()) == 18
    cells = {B * nx * ny for B, (nx, ny) in POOL_GRIDS.values()}
    reached |= {f"cells{c}" for c in cells}
    required = ({f"Q{q}" for q in (1, 3, 16, 32, 64)} | {"scalar-one-pass", "scalar-multi-pass", "C%4==0-above-256"}
                | {f"cells{c}" for c in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE)})
    assert not _unreached(required, reached), f"pooling paths no case reaches: {_unreached(required, reached)}"


def test_softmax_cases_reach_every_path():
    reached = set()
    for D in SOFTMAX_D:
        reached.add("reg" if softmax_reg(D) else "stream")
        reached |= {k for k, v in (("D=reg-limit", D == SM_SPLIT * SM_REG_BINS), ("D=reg-limit+1", D == SM_SPLIT * SM_REG_BINS + 1),
                                   ("D<waves", D < SM_SPLIT), ("idle-last-wave", softmax_chunk(D, 3)[0] >= D),
                                   ("ragged-chunks", D % SM_SPLIT != 0)) if v}
    reached |= {f"hw{'=' if hw == SM_PIX else ('<' if hw < SM_PIX else '>')}tile" for hw in SOFTMAX_HW}
    for name, (D, dt, d0, d1, keep) in SOFTMAX_INF.items():
        kind = "reg" if softmax_reg(D) else "stream"
        whole = [w for w in range(SM_SPLIT) if softmax_chunk(D, w)[0] < softmax_chunk(D, w)[1]
                 and d0 <= softmax_chunk(D, w)[0] and softmax_chunk(D, w)[1] <= d1
                 and not (keep is not None and softmax_chunk(D, w)[0] <= keep < softmax_chunk(D, w)[1])]
        assert whole, name
        reached.add(f"inf-chunk-{kind}-{DT_NAME[dt]}" if keep is None else f"single-finite-{kind}")
        if 0 in whole:
            reached.add(f"inf-first-chunk-{kind}")
    required = {"reg", "stream", "D=reg-limit", "D=reg-limit+1", "D<waves", "idle-last-wave", "ragged-chunks", "hw<tile",
                "hw=tile", "hw>tile", "inf-chunk-reg-f32", "inf-chunk-stream-f32", "inf-chunk-reg-bf16",
                "inf-chunk-stream-bf16", "single-finite-reg", "single-finite-stream", "inf-first-chunk-reg",
                "inf-first-chunk-stream"}
    assert not _unreached(required, reached), f"softmax paths no case reaches: {_unreached(required, reached)}"
    assert set(SOFTMAX_DTYPES) == {torch.float32, BF16} and {129, 200} <= set(SOFTMAX_D)    # bf16 on the streaming path


# ----------------------------------------------------------------------------------- the mirrors against the library
@pytest.fixture(scope="module")
def lib():
    from vampire_amd.build import build_library
    build_library(verbose=False)
    return _capi.load()


def _conv_desc(B, cin, cout, Z, Y, X):
    d = _capi.VampConvDesc()
    d.B, d.cin, d.cout, d.Z, d.Y, d.X = B, cin, cout, Z, Y, X
    return C.byref(d)


def test_conv3d_host_answers_match_the_mirror(lib):
    vols = [(1, 1, 1), (3, 4, 1), (2, 2, 3), (16, 11, 12), (257, 2, 4), (2, 3, 200), (1, 2, 192), (1, 2, 193), (1, 2, 384),
            (1, 2, 385), (16, 200, 200), (8, 100, 100), (1, 1, 256), (1, 1, 257), (1, 1, 300), (5, 7, 1024), (64, 512, 128),
            (1024, 1024, 16), (2048, 2048, 128)]
    n = 0
    for (Z, Y, X), B, cin, cout in itertools.product(vols, (1, 2, 7, 64), (16, 32, 8, 48), (16, 32, 0)):
        got = lib.vamp_conv3d_supported(_conv_desc(B, cin, cout, Z, Y, X))
        assert got == conv_supported(B, cin, cout, Z, Y, X), (B, cin, cout, Z, Y, X)
        assert lib.vamp_conv3d_workspace_bytes(_conv_desc(B, cin, cout, Z, Y, X)) == conv_workspace(B, cin, cout, Z, Y, X), \
            (B, cin, cout, Z, Y, X)
        n += got
    assert n > 100
    for bad in ((0, 16, 16, 1, 1, 1), (1, 16, 16, 0, 1, 1), (1, 16, 16, 1, 1, -4)):
        assert lib.vamp_conv3d_supported(_conv_desc(*bad)) == 0 and lib.vamp_conv3d_workspace_bytes(_conv_desc(*bad)) == 0
    for name, (cin, cout, (Z, Y, X), B, _) in CONV_CASES.items():
        assert lib.vamp_conv3d_supported(_conv_desc(B, cin, cout, Z, Y, X)) == 1, name


def test_conv3d_16bit_host_answers_match_the_mirror(lib):
    vols = [(1, 1, 8), (2, 3, 4), (2, 3, 6), (2, 3, 10), (2, 3, 12), (2, 3, 16), (13, 41, 8), (16, 200, 200), (64, 512, 512),
            (128, 512, 512), (256, 256, 256), (0, 3, 8), (2, 0, 8)]
    for (Z, Y, X), B, cin, cout in itertools.product(vols, (1, 3, 0), (0, 1, 8, 16, 17, 32, 33), (0, 1, 9, 16, 24, 32, 40)):
        d = (B, cin, cout, Z, Y, X)
        assert lib.vamp_conv3d_bf16_supported(_conv_desc(*d)) == conv16_supported(*d), d
        assert lib.vamp_conv3d_bf16_workspace_bytes(_conv_desc(*d)) == conv16_workspace(*d), d
    for cases in (CONV16_CASES, CONV16_REFUSED):
        for name, (cin, cout, (Z, Y, X), B) in cases.items():
            assert lib.vamp_conv3d_bf16_supported(_conv_desc(B, cin, cout, Z, Y, X)) == int(cases is CONV16_CASES), name


def test_gate_conv_host_answers_match_the_mirror(lib):
    n = 0
    for C_, oZ, cout in itertools.product(range(0, 42), range(0, 35), (0, 1, 15, 16, 17, 79, 80, 81, 200)):
        s = gc_shape(C_, oZ, cout)
        assert lib.vamp_gate_conv1x1_supported(C_, oZ, cout) == int(s is not None), (C_, oZ, cout)
        assert lib.vamp_gate_conv1x1_workspace_bytes(C_, oZ, cout) == gc_workspace(C_, oZ, cout), (C_, oZ, cout)
        n += s is not None
    assert n > 1000
    # the refusal says what the rule is
    x = (C.c_float * 4)()
    p = C.cast(x, C.c_void_p)
    assert lib.vamp_gate_conv1x1_forward(1, 7, 21, 16, 80, _capi.VAMP_DENSITY_SIGMOID, p, p, p, None, p, None) < 0
    msg = lib.vamp_last_error().decode()
    assert "not supported" in msg and "oZ <= 32" in msg and "oZ <= 20" in msg and "LDS" in msg, msg
    assert lib.vamp_gate_conv1x1_backward(1, 7, 21, 16, 80, _capi.VAMP_DENSITY_SIGMOID, p, p, p, p, p, p, p, None, p, 1 << 30,
                                          None) < 0
    assert "oZ <= 20" in lib.vamp_last_error().decode()


def test_resize_host_answers_match_the_mirror(lib):
    sizes = (0, 1, 2, 3, 4, 5, 7, 8, 13, 14, 15, 16, 50, 100, 200, 601, 1201)
    for i, o in itertools.product(sizes, sizes):
        for in3, out3 in (((i, 4, 4), (o, 4, 4)), ((4, i, 4), (4, o, 4)), ((4, 4, i), (4, 4, o)), ((i, i, i), (o, o, o))):
            assert lib.vamp_upsample_trilinear_supported(*in3, *out3) == resize_supported(in3, out3), (in3, out3)
        assert lib.vamp_upsample_trilinear_workspace_bytes(i, 5, 200) == resize_workspace((i, 5, 200))
    assert lib.vamp_upsample_trilinear_workspace_bytes(8, 100, 100) == (208 * 64 + 255) // 256 * 256
    for name, (B, C_, in3, out3) in RESIZE_CASES.items():
        assert lib.vamp_upsample_trilinear_supported(*in3, *out3) == 1, name
    assert lib.vamp_upsample_trilinear_supported(*RESIZE_REFUSED[2], *RESIZE_REFUSED[3]) == 0
    # the refusal is the backward's first answer: before any pointer is used, on a machine without a GPU
    x = (C.c_float * 4)()
    p = C.cast(x, C.c_void_p)
    assert lib.vamp_upsample_trilinear_backward_ex(1, 2, 2, 2, 8, 8, 8, _capi.VAMP_F32, p, p, p, 1 << 20, None) < 0
    assert "too large for the gather table" in lib.vamp_last_error().decode()


def test_pooling_host_answers_match_the_mirror(lib):
    grids = [(1, 1, 1), (16, 12, 1), (23, 89, 2), (32, 32, 3), (3, 683, 1), (128, 128, 1), (2047, 1, 1), (2048, 1, 1),
             (4096, 4096, 8), (46340, 46340, 1), (46341, 46341, 1), (0, 4, 1), (4, 4, 0)]
    for (nx, ny, nz), B, C_, P, code in itertools.product(grids, (1, 2, 4), (1, 80, 260, 0),
                                                          (1, 63, 473088, 1 << 30, (1 << 31) - 1, 0),
                                                          (_capi.VAMP_F32, _capi.VAMP_BF16, _capi.VAMP_F16)):
        d = _capi.VampPoolDesc(B, C_, P, nx, ny, nz, code)
        assert lib.vamp_voxel_pooling_workspace_bytes(C.byref(d)) == pool_workspace(B, C_, P, nx, ny, nz, code), \
            (B, C_, P, nx, ny, nz, code)
    assert pool_workspace(1, 80, 473088, 128, 128, 1, _capi.VAMP_F32) > 0 and pool_workspace(2, 8, 1 << 30, 4, 4, 1, 0) == 0


# ------------------------------------------------------------------------------------- the resize's table kernel in float32
def _axis_taps(n_in, n_out):
    """aten's taps of every output index in float32 (axis_scale / axis_tap of upsample.hip): i0, i1, l0, l1."""
    scale = f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    src = scale * np.arange(n_out, dtype=f32)
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(f32)
    return scale, i0, i1, l1.astype(f32), (f32(1) - l1).astype(f32)


def _axis_table(n_in, n_out):
    """upsample_axis_table_kernel for every source index at once: the outputs it visits from its start guess to its
    break, the slots it fills.  -> (begin [in], n [in] (unclamped), visited-and-hit mask [in, out], weights [in, out])"""
    scale, i0, i1, l1, l0 = _axis_taps(n_in, n_out)
    i = np.arange(n_in)[:, None]
    o = np.arange(n_out)[None, :]
    if scale > 0:
        with np.errstate(over="ignore"):
            start = np.maximum(0, (((i - 1).astype(f32) / scale).astype(np.int64) - 2))
    else:
        start = np.zeros_like(i)
    after = o >= start
    beyond = after & (i0[None, :] > i)
    brk = np.where(beyond.any(1), beyond.argmax(1), n_out)[:, None]
    hit = after & (o < brk) & ((i0[None, :] == i) | (i1[None, :] == i))
    w = (np.where(i0[None, :] == i, l0[None, :], f32(0)) + np.where(i1[None, :] == i, l1[None, :], f32(0))).astype(f32)
    return np.where(hit.any(1), hit.argmax(1), 0), hit.sum(1), hit, w


def test_resize_table_is_the_transpose_of_the_forward_taps():
    """For every in <= 48, out < 200 the library admits: the table the backward gathers through (start guess
    (i - 1) / scale - 2, break at the first floor(src) > i, `begin, n` as one contiguous run, 14 slots -- six in the
    kernel unrolled for six) holds exactly the forward's taps of every source index, transposed; and the forward's
    taps as a matrix reproduce F.interpolate."""
    pairs = 0
    for n_in, n_out in itertools.product(range(1, 49), range(1, 200)):
        if not run_fits(n_in, n_out):
            continue
        pairs += 1
        _, i0, i1, l1, l0 = _axis_taps(n_in, n_out)
        begin, n, hit, w = _axis_table(n_in, n_out)
        i = np.arange(n_in)[:, None]
        taps = (i0[None, :] == i) | (i1[None, :] == i)            # every output whose taps include i: the transpose
        assert (hit == taps).all(), f"{n_in} -> {n_out}: the table's walk misses or invents a hit"
        last = np.where(taps.any(1), n_out - 1 - taps[:, ::-1].argmax(1), -1)
        assert ((last - begin + 1 == n) | (n == 0)).all(), f"{n_in} -> {n_out}: hits are not one contiguous run"
        assert n.max() <= MAX_HITS, f"{n_in} -> {n_out}: {n.max()} hits"
        if run_fits(n_in, n_out, 6):
            assert n.max() <= 6, f"{n_in} -> {n_out}: {n.max()} hits in the kernel unrolled for six"
        # the weights: the transposed forward matrix, column sums one (every output's two taps)
        M = np.zeros((n_out, n_in), dtype=f32)
        np.add.at(M, (np.arange(n_out), i0), l0)
        np.add.at(M, (np.arange(n_out), i1), l1)
        assert (np.where(hit, w, 0).T == M).all(), f"{n_in} -> {n_out}: weights"
    assert pairs > 4000
    for n_in, n_out in ((2, 7), (1, 14), (3, 5), (9, 4), (48, 199), (5, 9), (7, 7), (4, 1)):
        _, i0, i1, l1, l0 = _axis_taps(n_in, n_out)
        x = torch.randn(1, 1, n_in, 1, 1, generator=gen(n_in * 1000 + n_out))
        ref = F.interpolate(x, (n_out, 1, 1), mode="trilinear", align_corners=True).flatten().numpy()
        mine = l0 * x.flatten().numpy()[i0] + l1 * x.flatten().numpy()[i1]
        assert np.abs(mine - ref).max() <= 1e-6, (n_in, n_out)
    # a ratio beyond the table would lose hits -- which is why it is refused
    assert not run_fits(2, 8) and _axis_table(2, 8)[1].max() == 8 and _axis_table(1, 15)[1].max() == 15


# ------------------------------------------------------------------------------------------------- the alignment guard
def test_alignment_guard_decides_on_the_first_byte():
    """Contiguous views that do not start on a 16-byte boundary are copied before their address reaches a kernel;
    aligned tensors pass as they are (no copy on the hot path)."""
    for dt, step in ((torch.float32, 4), (BF16, 2), (FP16, 2), (torch.int32, 4)):
        buf = torch.arange(64, dtype=torch.float32).to(dt)
        assert buf.data_ptr() % 16 == 0 and not _needs_aligned_copy(buf) and _aligned(buf) is buf
        for k in range(1, 16 // step):
            v = buf[k:k + 24].view(2, 3, 4)
            assert v.is_contiguous() and v.data_ptr() % 16 == k * step and _needs_aligned_copy(v)
            c = _aligned(v)
            assert c.data_ptr() % 16 == 0 and c.data_ptr() != v.data_ptr() and torch.equal(c, v) and c.is_contiguous()
        v = buf[16 // step:16 // step + 24]
        assert not _needs_aligned_copy(v) and _aligned(v) is v
    t = torch.arange(24.0).view(4, 6).t()                            # not contiguous: made contiguous (and aligned)
    c = _aligned(t)
    assert c.is_contiguous() and c.data_ptr() % 16 == 0 and torch.equal(c, t)
