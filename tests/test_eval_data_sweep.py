"""The scoring and data-side kernels across the sizes that pick their code paths -- seg_metrics.hip (confusion matrix,
lidar-seg prediction), camera_images.hip, point_queries.hip and det_eval.hip -- with the oracles, input builders,
comparison helpers and bars of the kernels' own test modules (test_seg_metrics, test_camera_images, test_point_queries
and through it test_sample_points_sweep, test_det_eval), none of them restated or loosened: every case here is a shape,
a placement or a value those modules do not run.

confusion    element counts that fill the 1024-workgroup grid exactly once, once plus one lane group, and three times
             (rows mode) and twice in the 4-wide planes mode, with whole waves masked out or ignored in one trip and live
             in the other; Kc = 32 (1025 bins) and Kc = 1; class windows of width 1, 8, 9, 10, 18, 19 and 27 inside
             (0, K) with NaNs on class hi - 1 and all-(-inf) windows; the three target types with and without a mask
             under the vector loads; pred, target or mask off its vector alignment; two calls into one state.
lidar-seg    R = 2047 / 2048 / 2049 / 4097 (one, two, two and three scan tiles of R + 1 runs), windows of 64 classes
             and of one, a run of 300 points between empty runs, every index out of range, bf16 logits.  Bit-exact.
images       raw 130 x 340 at the smallest resize the plan accepts (0.254: all 16 taps, a 44 x 265 footprint under a tile)
             and at 0.27 (15 taps, 41 x 250), with flips, +-5.4 degree rotations and a crop that overruns on the left
             and at the bottom; upscales 2 and 3;
             W = 1, 3, 5, 64, 128 and H = 1, 7, 8, 9, 16; bf16 with W % 4 != 0; the uint8 image alone; raw rows that
             start on each of the four byte phases.
queries      the backward at every CP4 the feature test leaves out (K = 4, 8, 12, 20, 24), K + 1 a whole number of
             quads (7, 11, 15) and K = 1, each on the crowded scene (the 8-lane gather and the 64-lane heavy kernel);
             X = 5, 32, 65, Y = 1, Z = 1; sigmoid density; bf16 density; no lidar set, no occupancy set, no sdf, a shared
             grid, upstream gradients for two outputs only; a sample with count 0 between two live ones.
det_eval     ground truth of one class in one sample at 2 ... 255 boxes (every lane count of the walk from 1 to 64,
             ragged last lanes), G = 600 and 1100 with the class interleaved with others and padding (three and five
             trips of the compaction), M = 513 and 2048, 16 classes, nearest boxes tied across two lanes and across two
             registers of a lane at each threshold (which box was taken shows at the first three), non-finite centres, and scores that are negative, -0.0 beside
             +0.0, +-inf, fp16 subnormals and NaNs of either sign and with a payload, in fp32, bf16 and fp16.

The CPU tests at the end mirror the host formulas that choose these paths, map every GPU case through them and fail
with the name of any listed regime that no case reaches, and compare the mirrors with the library's *_workspace_bytes /
*_record_bytes over grids of descriptors that include sizes no GPU test could allocate.

Found here: det_eval's score key gave a NaN with the sign bit set the lowest place of its class where the header and
the host's sort give it the highest, and let two NaNs of different payload differ; ev_key now gives every NaN the one
key above +inf's.

Measured on an MI355X: the 90 GPU tests of this file take 5 s in all; the slowest single case is the first point-query
case (K4, 1.3 s with the first float64 reference and the library's load), and no other case takes more than 0.35 s.
Largest fraction of a gradient bar over the 22 point-query cases: against float64 grad_semantic 0.26 (K24),
grad_density 0.16 (no-occupancy), grad_beta 0.27 (bf16-density); against the existing calls grad_semantic 0.27 (K15),
grad_density 0.071 (Z1), grad_beta 0.27 (no-lidar)."""
import ctypes as C
import dataclasses
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import test_camera_images as TI
import test_det_eval as TE
import test_point_queries as TQ
import test_seg_metrics as TM
from vampire_amd import _capi, metrics, ops
from vampire_amd import images as I
from test_seg_metrics import dev  # noqa: F401  (the module-scoped device fixture)

gpu = pytest.mark.gpu
I31 = 0x7fffffff
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cdiv(a, b):
    return -(-a // b)


def align_up(v, a):
    return cdiv(v, a) * a


def _unreached(required, reached):
    return sorted(str(r) for r in set(required) - set(reached))


# =====================================================================================================================
# confusion matrix: mirrors, cases, inputs
# =====================================================================================================================
CONF_BLOCK, CONF_MAX_GRID, CONF_BATCH, CONF_MAX_KC = 256, 1024, 9, 32
CONF_STRIDE = CONF_BLOCK * CONF_MAX_GRID                   # lane groups of one trip of a full grid
T_ALIGN = {torch.int64: 16, torch.int32: 16, torch.uint8: 4}
T_CODE = {torch.int64: _capi.VAMP_I64, torch.int32: _capi.VAMP_I32, torch.uint8: _capi.VAMP_U8}


def conf_mode(layout, S, misaligned):
    """ROWS, PLANES or PLANES4 (four neighbouring elements of a class plane per lane): S % 4 and every pointer aligned."""
    if layout == "rows":
        return "rows"
    return "planes4" if S % 4 == 0 and misaligned is None else "planes"


def conf_grid(n, V):
    return min(cdiv(n // V, CONF_BLOCK), CONF_MAX_GRID)


def conf_trips(n, V):
    """(trips of workgroup 0 through the grid-stride loop, lane groups of its last trip over the whole grid)."""
    groups, stride = n // V, conf_grid(n, V) * CONF_BLOCK
    trips = cdiv(groups, stride)
    return trips, groups - (trips - 1) * stride


def conf_batches(lo, hi):
    """(class batches of nine, classes the last batch re-reads as class hi - 1)."""
    nb = cdiv(hi - lo, CONF_BATCH)
    return nb, nb * CONF_BATCH - (hi - lo)


def conf_valid(B, S, K, layout, pdt, tdt, Kc, lo, hi):
    if not (0 <= B < I31 and 0 <= S < I31 and B * S < I31 and 1 <= Kc <= CONF_MAX_KC and tdt in T_CODE.values()):
        return False
    if pdt in (_capi.VAMP_I64, _capi.VAMP_I32):
        return layout == _capi.VAMP_SEG_ROWS and K == 1
    return (pdt in (_capi.VAMP_F32, _capi.VAMP_BF16) and layout in (_capi.VAMP_SEG_ROWS, _capi.VAMP_SEG_PLANES)
            and 1 <= K < 0x10000 and 0 <= lo < hi <= K and hi - 1 < Kc)


def conf_workspace(B, S, K, layout, pdt, tdt, Kc, lo, hi):
    if not conf_valid(B, S, K, layout, pdt, tdt, Kc, lo, hi):
        return 0
    return max(conf_grid(B * S, 1), 1) * (Kc * Kc + 1) * 4


@dataclasses.dataclass(frozen=True)
class ConfCase:
    layout: str                     # "rows" | "planes" ([B, K, S] memory behind a permute view)
    B: int
    S: int
    K: int
    Kc: int = None                  # default K
    window: tuple = None
    tdtype: torch.dtype = torch.int64
    mask: bool = False
    ignore: int = None
    misaligned: str = None          # "pred" | "target" | "mask": that tensor starts one element into its buffer
    dead: tuple = ()                # (first lane group, lane groups, "mask" | "ignore"): made dead that way
    calls: int = 1

    @property
    def n(self):
        return self.B * self.S

    @property
    def kc(self):
        return self.Kc or self.K


W_K, W_LO = 30, 2
CONF_CASES = {
    "rows-one-trip": ConfCase("rows", 1, CONF_STRIDE, 3),
    "rows-one-trip+1": ConfCase("rows", 1, CONF_STRIDE + 1, 3, tdtype=torch.uint8),
    "rows-three-trips": ConfCase("rows", 1, 2 * CONF_STRIDE + 1, 3, mask=True,
                                 dead=((64, 64, "mask"), (CONF_STRIDE + 128, 64, "mask"))),
    "planes4-two-trips": ConfCase("planes", 5, (4 * CONF_STRIDE + 4) // 5, 2, ignore=1, tdtype=torch.int32,
                                  dead=((0, 64, "ignore"),)),
    "Kc32": ConfCase("rows", 1, 4001, 32),
    "Kc1": ConfCase("rows", 1, 300, 1),
    "two-calls": ConfCase("rows", 1, 5000, 6, mask=True, calls=2),
}
for _i, _w in enumerate((1, 8, 9, 10, 18, 19, 27)):
    CONF_CASES[f"window-w{_w}"] = ConfCase(("rows", "planes")[_i % 2], 2, 1003, W_K, Kc=W_K - 1, window=(W_LO, W_LO + _w),
                                           tdtype=(torch.int64, torch.uint8, torch.int32)[_i % 3], mask=_i % 2 == 0, ignore=3)
for _t, _m in itertools.product(T_CODE, (False, True)):
    CONF_CASES[f"planes4-{str(_t)[6:]}-{'mask' if _m else 'nomask'}"] = ConfCase("planes", 2, 1000, 5, tdtype=_t, mask=_m)
for _which in ("pred", "target", "mask"):
    CONF_CASES[f"misaligned-{_which}"] = ConfCase("planes", 2, 1000, 5, mask=True, misaligned=_which)


@functools.lru_cache(maxsize=None)
def conf_inputs(name):
    """Per call (logits [B, S, K] fp32 with ties, target [B, S], mask [B, S] | None), CPU.  Window cases carry NaNs on
    class hi - 1 (the class the last batch re-reads), NaNs outside the window and windows that are all -inf."""
    c = CONF_CASES[name]
    g = gen(1000 + list(CONF_CASES).index(name))
    calls = []
    for _ in range(c.calls):
        x = (torch.randn(c.B, c.S, c.K, generator=g) * 2).round() / 2
        t = torch.randint(0, c.kc, (c.B, c.S), generator=g)
        if c.n >= 100:
            t[0, 5:8] = c.kc                                                  # out of range: counted as invalid
        m = (torch.rand(c.B, c.S, generator=g) < 0.7) if c.mask else None
        if c.window:
            lo, hi = c.window
            x[:, 0:10, hi - 1] = float("nan")
            x[:, 10:20, lo:hi] = float("-inf")
            x[:, 20:30, hi:] = float("nan")
            x[:, 20:30, :lo] = float("inf")
            if m is not None:
                m[:, :30:2] = True
        V = 4 if conf_mode(c.layout, c.S, c.misaligned) == "planes4" else 1
        for g0, ng, how in c.dead:
            sl = slice(g0 * V, (g0 + ng) * V)
            if how == "mask":
                m.view(-1)[sl] = False
            else:
                t.view(-1)[sl] = c.ignore
        calls.append((x, t.to(c.tdtype), m))
    return calls


def conf_live_groups(name):
    """[lane groups] bool: the group has an element that is counted (mask true and target not ignored)."""
    c = CONF_CASES[name]
    x, t, m = conf_inputs(name)[0]
    live = torch.ones(c.n, dtype=torch.bool) if m is None else m.reshape(-1).clone()
    if c.ignore is not None:
        live &= t.reshape(-1).long() != c.ignore
    V = 4 if conf_mode(c.layout, c.S, c.misaligned) == "planes4" else 1
    return live.view(-1, V).any(1)


def offset_copy(t, dev):
    """`t` on the device, starting one element into a buffer of its own."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def conf_place(c, x, t, m, dev):
    """The device tensors of one call in the case's layout and alignment."""
    put = lambda v, which: offset_copy(v, dev) if c.misaligned == which else v.to(dev)
    if c.layout == "rows":
        xd = put(x.reshape(-1, c.K), "pred")
        td, md = put(t.reshape(-1), "target"), None if m is None else put(m.reshape(-1), "mask")
    else:
        xd = put(x.permute(0, 2, 1).contiguous(), "pred").permute(0, 2, 1)                 # [B, S, K] over [B, K, S]
        td, md = put(t, "target"), None if m is None else put(m, "mask")
        assert not xd.is_contiguous()
    for v, a, which in ((xd, 16, "pred"), (td, T_ALIGN[c.tdtype], "target"), (md, 4, "mask")):
        if v is not None:
            assert (v.data_ptr() % a != 0) == (c.misaligned == which), (which, v.data_ptr())
    return xd, td, md


@gpu
@pytest.mark.parametrize("name", list(CONF_CASES))
def test_confusion_paths(dev, name):
    """Counts and the invalid counter equal to test_seg_metrics.ref_confmat, summed over the case's calls."""
    c = CONF_CASES[name]
    cm = torch.zeros(c.kc, c.kc, dtype=torch.int64, device=dev)
    inv = torch.zeros((), dtype=torch.int64, device=dev)
    want, want_inv = torch.zeros(c.kc, c.kc, dtype=torch.int64), 0
    for x, t, m in conf_inputs(name):
        xd, td, md = conf_place(c, x, t, m, dev)
        TM._run(xd, td, md, c.window, c.ignore, state=(cm, inv))
        rcm, rinv = TM.ref_confmat(x.reshape(-1, c.K), t.reshape(-1), None if m is None else m.reshape(-1), c.window,
                                   c.kc, c.ignore)
        want, want_inv = want + rcm, want_inv + rinv
    V = 4 if conf_mode(c.layout, c.S, c.misaligned) == "planes4" else 1
    print(f"[confusion:{name}] mode {conf_mode(c.layout, c.S, c.misaligned)}, grid {conf_grid(c.n, V)}, trips "
          f"{conf_trips(c.n, V)}, counted {int(want.sum())}, invalid {want_inv}, differing bins "
          f"{int((cm.cpu() != want).sum())}")
    assert torch.equal(cm.cpu(), want), (cm.cpu() - want).abs().max()
    assert int(inv) == want_inv
    assert int(want.sum()) > 0


# =====================================================================================================================
# lidar-seg prediction
# =====================================================================================================================
SCAN_TILE, SCAN_PAD = 2048, 64


def ls_tiles(R):
    return align_up(R + 1, SCAN_TILE) // SCAN_TILE


def ls_workspace(P, R):
    if not (0 <= P < I31 and 0 <= R < I31 - 2 * SCAN_TILE):
        return 0
    ncell, nt = ls_tiles(R) * SCAN_TILE, ls_tiles(R)
    return sum(align_up(n, 256) for n in ((ncell + SCAN_PAD + 1) * 4, ncell * 4, nt * 4, nt * 4, (nt + 4) * 4,
                                          max(P, 1) * 4, max(P, 1) * 4))


@dataclasses.dataclass(frozen=True)
class LsCase:
    P: int
    R: int
    K: int = 18
    window: tuple = (1, 17)
    dtype: torch.dtype = F32
    scene: str = "random"           # "random" | "long-run" | "all-out"


LS_CASES = {f"R{r}": LsCase(3000, r) for r in (2047, 2048, 2049, 4097)}
LS_CASES.update({
    "window-64": LsCase(400, 50, K=66, window=(1, 65)),
    "window-1": LsCase(400, 50, K=6, window=(3, 4)),
    "long-run": LsCase(700, 40, scene="long-run"),
    "all-out-of-range": LsCase(100, 10, scene="all-out"),
    "bf16": LsCase(2000, 600, dtype=BF16),
})
LS_LONG = (5, 300)                  # the reference point of the long run and its points


@functools.lru_cache(maxsize=None)
def ls_inputs(name):
    c = LS_CASES[name]
    g = gen(c.P + c.R)
    logits = (torch.randn(c.P, c.K, generator=g) * 10).to(c.dtype)
    idx = torch.randint(0, c.R, (c.P,), generator=g)
    idx[: c.P // 3] = idx[c.P // 3: 2 * (c.P // 3)].flip(0)                      # repeats, out of point order
    if c.scene == "long-run":
        r, n = LS_LONG
        idx = torch.where((idx >= r - 1) & (idx <= r + 1), torch.full_like(idx, r + 2), idx)
        idx[torch.randperm(c.P, generator=g)[:n]] = r
    elif c.scene == "all-out":
        idx = torch.tensor([-1, c.R, c.R + 100, -(1 << 40)])[torch.randint(0, 4, (c.P,), generator=g)]
    return logits, idx


@gpu
@pytest.mark.parametrize("name", list(LS_CASES))
def test_lidarseg_paths(dev, name):
    """Labels bit-exact against test_seg_metrics.ref_lidarseg_labels (a sequential CPU index_add_) on the points whose
    index is in range; the others are counted."""
    c = LS_CASES[name]
    logits, idx = ls_inputs(name)
    labels, inv = ops.lidarseg_predict(logits.to(dev), idx.to(dev), c.R, c.window)
    keep = (idx >= 0) & (idx < c.R)
    want = TM.ref_lidarseg_labels(logits[keep], idx[keep], c.R, *c.window)
    print(f"[lidarseg:{name}] P {c.P}, R {c.R}, scan tiles {ls_tiles(c.R)}, out of range {int((~keep).sum())}, longest run "
          f"{int(torch.bincount(idx[keep], minlength=1).max()) if bool(keep.any()) else 0}, differing labels "
          f"{int((labels.cpu() != want).sum())}")
    assert labels.shape == (c.R,) and labels.dtype == torch.int64
    assert int(inv) == int((~keep).sum())
    assert torch.equal(labels.cpu(), want)
    if c.scene == "all-out":
        assert bool((labels == c.window[0]).all())
    else:
        assert len(torch.unique(want)) > 1 or c.window[1] - c.window[0] == 1


# =====================================================================================================================
# camera images
# =====================================================================================================================
IMG_TW, IMG_TH, IMG_K = _capi.VAMP_IMG_TILE_W, _capi.VAMP_IMG_TILE_H, _capi.VAMP_IMG_MAX_TAPS
IMG_HROW = IMG_TW * 3
CORNER_RAW, CORNER_RESIZE = (130, 340), 0.254       # the smallest resize (to 0.001) the plan accepts for this raw size


def img_raw_pitch(foot_w):
    p = align_up(foot_w * 3 + 3, 4)
    return p + 4 if (p // 4) % 2 == 0 else p


def img_lds(foot_w, foot_h):
    return foot_h * (IMG_HROW + img_raw_pitch(foot_w))


def img_valid(d):
    return (1 <= d.B <= 4096 and 1 <= d.N <= 16 and 1 <= d.raw_h <= 65536 and 1 <= d.raw_w <= 65536
            and 1 <= d.H <= 4096 and 1 <= d.W <= 4096 and 1 <= d.taps_x <= IMG_K and 1 <= d.taps_y <= IMG_K
            and 1 <= d.foot_w <= _capi.VAMP_IMG_FOOT_W and 1 <= d.foot_h <= _capi.VAMP_IMG_FOOT_H
            and d.out_dtype in (_capi.VAMP_F32, _capi.VAMP_BF16, _capi.VAMP_IMG_OUT_NONE) and d.to_rgb in (0, 1)
            and d.raw_row_stride >= d.raw_w * 3 and d.raw_n_stride >= 0 and d.raw_b_stride >= 0 and d.B * d.N <= 65535)


def img_workspace(d):
    return align_up(d.B * d.N * d.H * align_up(d.W * 3, 16), 256) if img_valid(d) else 0


@dataclasses.dataclass(frozen=True)
class ImgCase:
    raw_hw: tuple
    final: tuple
    resize: float
    dtype: object = F32             # torch.float32 | torch.bfloat16 | None (the uint8 image alone)
    pad_w: int = 0                  # raw sits in a buffer this many pixels wider, one pixel in
    to_rgb: bool = True


IMG_CASES = {
    "corner-18x70": ImgCase(CORNER_RAW, (18, 70), CORNER_RESIZE),
    "corner-20x44": ImgCase(CORNER_RAW, (20, 44), CORNER_RESIZE, to_rgb=False),
    "resize0.27-18x70": ImgCase(CORNER_RAW, (18, 70), 0.27),
    "up2-20x44": ImgCase((16, 24), (20, 44), 2.0),
    "up3-20x44": ImgCase((16, 24), (20, 44), 3.0),
    "1x1": ImgCase((37, 53), (1, 1), 0.55),
    "7x3": ImgCase((37, 53), (7, 3), 0.55),
    "8x5": ImgCase((37, 53), (8, 5), 0.55),
    "9x64": ImgCase((64, 96), (9, 64), 1.0),
    "16x128": ImgCase((64, 96), (16, 128), 1.4),
    "bf16-18x70": ImgCase((64, 96), (18, 70), 0.8, dtype=BF16),
    "u8-alone-9x5": ImgCase((37, 53), (9, 5), 0.44, dtype=None),
    "row-phases": ImgCase((37, 53), (20, 44), 1.0, pad_w=2),
}


def img_augs(c):
    """One sample, six cameras: every (rotate, flip) of test_camera_images.ROTATES; the crops alternate between a window
    inside the resized image (where it fits), one that overruns it on the left and at the bottom, and the feature
    sweep's overrun on the right and at the top."""
    H, W = c.final
    new_w, new_h = int(c.raw_hw[1] * c.resize), int(c.raw_hw[0] * c.resize)
    row = []
    for i, (rotate, flip) in enumerate(itertools.product(TI.ROTATES, (False, True))):
        if i % 3 == 0:
            x0, y0 = max(0, (new_w - W) // 2), max(0, new_h - H)
        elif i % 3 == 1:
            x0, y0 = -5, new_h - H + 3
        else:
            x0, y0 = new_w - W + 5, -3
        row.append(TI.tup(c.raw_hw, c.resize, x0, y0, c.final, flip, rotate))
    return [row]


@functools.lru_cache(maxsize=None)
def img_plan(name):
    c = IMG_CASES[name]
    return I.plan_camera_images(img_augs(c), c.raw_hw, c.final)


def img_taps(plan):
    return int(plan.col_count.max()), int(plan.row_count.max())


def img_row_stride(c):
    return 3 * (c.raw_hw[1] + c.pad_w)


@gpu
@pytest.mark.parametrize("name", list(IMG_CASES))
def test_camera_image_paths(dev, name):
    """The uint8 image and its normalisation equal to test_camera_images.apply_plan / assert_images."""
    c = IMG_CASES[name]
    plan = img_plan(name)
    raw = TI.raw_frames(1, 6, *c.raw_hw)
    want = TI.oracle_u8(raw, plan)
    rd = torch.from_numpy(raw).to(dev)
    if c.pad_w:
        h, w = c.raw_hw
        big = torch.full((1, 6, h, w + c.pad_w, 3), 0xEE, dtype=torch.uint8, device=dev)
        big[:, :, :, 1:1 + w] = rd
        rd = big[:, :, :, 1:1 + w]
        assert rd.stride(2) == img_row_stride(c) and {(rd.data_ptr() + r * rd.stride(2)) % 4 for r in range(h)} == {0, 1, 2, 3}
    print(f"[images:{name}] raw {c.raw_hw} -> {c.final} at {c.resize}: taps {img_taps(plan)}, footprint {plan.foot_h} x "
          f"{plan.foot_w}, LDS {img_lds(plan.foot_w, plan.foot_h)} bytes, non-zero bytes {int((want != 0).sum())} of {want.size}")
    assert want.any()
    if c.dtype is None:
        out, u8 = I.camera_images(rd, plan.to(dev), dtype=None, out_u8=True)
        assert out is None and torch.equal(u8.cpu(), torch.from_numpy(want))
        return
    out, u8 = I.camera_images(rd, plan.to(dev), to_rgb=c.to_rgb, dtype=c.dtype, out_u8=True)
    assert out.dtype == c.dtype
    TI.assert_images(out, u8, want, c.to_rgb, name)


# =====================================================================================================================
# point queries
# =====================================================================================================================
PQ_PVPB, PQ_HEAVY, PQ_HEAVY_GRID = 32, 256, 4096


def pq_cp(K):
    """(CP: the gradient row's width, CP4: the instantiation, pad columns)."""
    cp = align_up(K + 1, 4)
    return cp, cp // 4, cp - (K + 1)


def pq_workspace(B, K, Z, Y, X, M, P):
    from vampire_amd.queries import point_queries_supported
    if not point_queries_supported(B, K, Z, Y, X, M, P):
        return 0
    ncell = align_up(B * (Z + 1) * (Y + 1) * (X + 1) + 2, SCAN_TILE)
    nt, src, vox = ncell // SCAN_TILE, B * (M + 2 * P), B * Z * Y * X
    nblk = cdiv(X, PQ_PVPB) * Y * Z * B
    return sum(align_up(n, 256) for n in ((ncell + SCAN_PAD) * 4, ncell * 4, nt * 4, nt * 4, (nt + 4) * 4, vox * 4, src * 4,
                                          src * 4, src * 16, src * 16, src * pq_cp(K)[0] * 4, (nblk + PQ_HEAVY_GRID) * 4))


@dataclasses.dataclass(frozen=True)
class PqCase:
    K: int
    X: int = 33
    Y: int = 16
    Z: int = 5
    mode: str = "sdf"
    lidar: bool = True
    occupancy: bool = True
    sdf: bool = True
    shared: bool = False
    given: tuple = (True, True, True, True)
    den_dtype: torch.dtype = F32
    sites: tuple = ((4, 2, 2), (20, 9, 2))
    zero_between: bool = False      # the counts are [n0, 0, n1] instead of [n0, n1, 0]


PQ_CASES = {f"K{k}": PqCase(k) for k in (4, 8, 12, 20, 24, 7, 11, 15, 1)}
PQ_CASES.update({
    "X5": PqCase(3, X=5, sites=((2, 4, 2), (2, 10, 2))),
    "X32": PqCase(3, X=32),
    "X65": PqCase(3, X=65),
    "Y1": PqCase(3, Y=1, sites=((4, 0, 2), (20, 0, 2))),
    "Z1": PqCase(3, Z=1, sites=((4, 2, 0), (20, 9, 0))),
    "naive": PqCase(3, mode="naive", sdf=False),
    "bf16-density": PqCase(3, den_dtype=BF16),
    "no-lidar": PqCase(3, lidar=False),
    "no-occupancy": PqCase(3, occupancy=False),
    "no-sdf": PqCase(3, sdf=False),
    "shared-grid": PqCase(3, shared=True),
    "upstream-for-two": PqCase(3, given=(True, False, False, True)),
    "count-0-between": PqCase(3, zero_between=True),
})


def pq_case(c):
    return dataclasses.replace(TQ.qcase(c.K, c.X, 3, c.mode, 0.1), Y=c.Y, Z=c.Z)


@functools.lru_cache(maxsize=None)
def pq_scene(name):
    """test_point_queries.crowded_scene at the case's sites; `zero_between` swaps samples 1 and 2 of the lidar set."""
    c = PQ_CASES[name]
    pts, counts, occ, sites = TQ.crowded_scene(pq_case(c), c.sites)
    if c.zero_between:
        pts, counts = pts[[0, 2, 1]], [counts[0], 0, counts[1]]
    return pts, counts, occ, sites


def pq_union_records(name):
    """[B, Z, Y, X]: the records of each voxel's list in the backward -- live lidar rows and occupancy points through
    the clipped taps, and the occupancy points outside the bounds once more through the unclipped ones."""
    c = PQ_CASES[name]
    case = pq_case(c)
    pts, counts, occ, _ = pq_scene(name)
    n = torch.zeros(3, c.Z, c.Y, c.X, dtype=torch.int64)
    if c.lidar:
        n += torch.cat([TQ.voxel_records(case.cfg, pts[b:b + 1, :k], True, False) for b, k in enumerate(counts)])
    if c.occupancy:
        o = (occ[:1] if c.shared else occ).expand(3, -1, -1)
        inside = inside_bounds(case.cfg, o)
        n += TQ.voxel_records(case.cfg, o, True, False)
        n += TQ.voxel_records(case.cfg, torch.where(inside[..., None], torch.full_like(o, float("nan")), o), False, False)
    return n


def inside_bounds(cfg, pts):
    """[..] bool: the point lies inside the bounds on all three axes (test_sample_points_sweep.taps)."""
    from test_sample_points_sweep import taps
    return taps(cfg, pts, False)[2]


@gpu
@pytest.mark.parametrize("name", list(PQ_CASES))
def test_point_query_paths(dev, name):
    """The forward torch.equal to the existing calls on the parts asked for, then test_point_queries.gradient_check:
    the fused backward against float64 and against the existing calls at the sum of the parts' bars (part_bar,
    ACT_GRAD_BAR, ACT_BETA_BAR), unchanged."""
    c = PQ_CASES[name]
    case = pq_case(c)
    pts, counts, occ, _ = pq_scene(name)
    hp = TQ.shared_hot(case.cfg, dev)
    sem, den = (v.to(dev) for v in TQ.volumes(case))
    den = den.to(c.den_dtype)
    occ_d = (occ[:1] if c.shared else occ).to(dev)
    occ_b = occ_d.expand(3, -1, -1).contiguous()
    bt = TQ.beta_of(case, dev)
    kw = {}
    if c.lidar:
        kw.update(points=pts.to(dev), counts=torch.tensor(counts, dtype=torch.int32, device=dev), sdf=c.sdf)
    if c.occupancy:
        kw.update(occ_points=occ_d)
    with torch.no_grad():
        q = hp.point_queries(sem, den, bt if c.occupancy else None, **kw)
        pl, ps, ol, od = TQ.split_calls(hp, case, sem, den, bt, pts.to(dev), counts, occ_b, c.sdf)
    assert (q.pts_logits is not None) == c.lidar and (q.pts_sdf is not None) == (c.lidar and c.sdf)
    assert (q.occ_logits is not None) == c.occupancy == (q.occ_density is not None)
    if c.lidar:
        TQ.assert_rows(q.pts_logits, pl, counts, "pts_logits")
        if c.sdf:
            TQ.assert_rows(q.pts_sdf, ps, counts, "pts_sdf")
    if c.occupancy:
        assert torch.equal(q.occ_logits, ol) and torch.equal(q.occ_density, od)
    seen, n_l, n_o = TQ.gradient_check(dev, case, (pts, counts, occ, c.sites), lidar=c.lidar, occupancy=c.occupancy,
                                       sdf=c.sdf, shared=c.shared, given=c.given, den_dtype=c.den_dtype, tag=f"sweep {name}")
    worst = {}
    for (ref, what), e in seen.items():
        worst[what] = max(worst.get(what, 0.0), e)
    print(f"[queries:{name}] CP {pq_cp(c.K)}, runs_x {cdiv(c.X, PQ_PVPB)}, largest fraction of the bar: "
          + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    if c.lidar:
        zero = counts.index(0)
        assert int(n_l[zero].sum()) == 0 and all(int(n_l[b].sum()) > 0 for b in range(3) if b != zero)


# =====================================================================================================================
# detection scoring
# =====================================================================================================================
EV_BLOCK, EV_GT_CAP, EV_PER_LANE = 256, TE.GT_CAP, TE.GT_CAP // 64
NAMES16 = TE.NAMES + TE.NAMES[:6]
PED, CAR = TE.PED, TE.CAR
GT_SIZES = (2, 4, 5, 8, 9, 16, 17, 32, 33, 128, 129, 255)
BIG = dict(max_boxes_per_sample=2048)


def ev_act(ngc):
    """The walk's lane count: the lanes that hold ground truth, four boxes each, rounded up to a power of two."""
    act = 1
    while act * EV_PER_LANE < ngc:
        act <<= 1
    return act


def ev_record_bytes(d):
    ok = (1 <= d.B <= 4096 and 1 <= d.M <= _capi.VAMP_DET_EVAL_MAX_WIDTH and 0 <= d.G <= 1 << 20 and d.box_cols in (7, 9)
          and 1 <= d.num_classes <= _capi.VAMP_DET_EVAL_MAX_CLASSES and d.max_boxes_per_sample >= 1
          and d.max_samples >= 1 and d.max_samples * d.M < 1 << 31)
    return d.max_samples * d.M * _capi.VAMP_DET_EVAL_RECORD_BYTES if ok else 0


def survivors(samples, cls, names=TE.NAMES):
    """Per sample (ground truth, predictions) of class `cls` inside its range: the oracle's filter."""
    out = []
    for s in samples:
        inr = lambda b: np.sqrt(b[:, 0].astype(np.float64) ** 2 + b[:, 1].astype(np.float64) ** 2) < TE.RANGE[names[cls]]
        out.append((int(((s["gt_labels"] == cls) & inr(s["gt_boxes"])).sum()), int(((s["labels"] == cls) & inr(s["boxes"])).sum())))
    return out


def interleaved(G, n_pred, seed):
    """One sample with G ground-truth rows: pedestrians on every fifth row, cars on the next, padding rows (label -1)
    and four other classes between them; the predictions aim at the pedestrians and cars."""
    rng = np.random.default_rng(seed)
    s = TE.random_scene(rng, G, n_pred, [PED], spread=20.0, on_ranges=False)
    others = [-1, TE.BUS, -1, TE.BICYCLE, TE.CONE, -1, TE.BARRIER, -1]
    lab = np.array([PED if i % 5 == 0 else CAR if i % 5 == 1 else others[i % 8] for i in range(G)], dtype=np.int64)
    src = rng.integers(0, G // 5, n_pred) * 5 + rng.integers(0, 2, n_pred)
    boxes = s["boxes"].copy()
    boxes[:, :2] = s["gt_boxes"][src, :2] + TE.q64(rng, -1, 1, (n_pred, 2))
    return dict(s, gt_labels=lab, labels=lab[src], boxes=boxes)


def tie_scene(same_lane):
    """Four places 12 m apart, one per threshold: two pedestrians the same distance d either side of a prediction, d
    inside (th[h - 1], th[h]); a second prediction of lower score there takes the other one.  The two boxes of a place
    are rows j and j + 4 (two lanes of the walk) or rows 2 j and 2 j + 1 (two registers of one lane); the lower row has
    other sizes, so that the scale error tells which one was taken."""
    ds = (0.25, 0.75, 1.5, 3.0)
    gt = [None] * 8
    preds, scores = [], []
    for j, d in enumerate(ds):
        lo, hi = (2 * j, 2 * j + 1) if same_lane else (j, j + 4)
        cx = 12.0 * j - 18.0
        gt[lo] = TE.box(cx - d, 1.0, dims=(1.0, 1.0, 1.0))
        gt[hi] = TE.box(cx + d, 1.0)
        preds += [TE.box(cx, 1.0, yaw=0.5), TE.box(cx, 1.0, yaw=-0.5)]
        scores += [(200 - j) / 256, (100 - j) / 256]
    return TE.sample(preds, scores, [PED] * 8, gt, [PED] * 8)


def nonfinite_scene():
    """Predictions and ground truth whose centre is NaN or +-inf in x or y, between finite ones that match."""
    nan, inf = float("nan"), float("inf")
    bad = [(nan, 1.0), (1.0, nan), (inf, 1.0), (1.0, -inf), (-inf, inf), (nan, nan)]
    gt = [TE.box(6.0 * i - 15.0, 2.0) for i in range(6)]
    preds = [TE.box(6.0 * i - 14.75, 2.0) for i in range(6)]
    for i, (x, y) in enumerate(bad):
        gt.insert(2 * i, TE.box(x, y))
        preds.insert(2 * i + 1, TE.box(x, y))
    n = len(preds)
    return TE.sample(preds, [(200 - i) / 256 for i in range(n)], [CAR] * n, gt, [CAR] * len(gt))


# score bit patterns per type: (fp32, bf16, fp16)
SCORE_BITS = {
    "-0.5": (0xBF000000, 0xBF00, 0xB800), "-0": (0x80000000, 0x8000, 0x8000), "+0": (0, 0, 0),
    "+inf": (0x7F800000, 0x7F80, 0x7C00), "-inf": (0xFF800000, 0xFF80, 0xFC00), "1": (0x3F800000, 0x3F80, 0x3C00),
    "2^-24": (0x33800000, 0x3380, 0x0001), "2^-23": (0x34000000, 0x3400, 0x0002), "-2^-24": (0xB3800000, 0xB380, 0x8001),
    "nan+": (0x7FC00000, 0x7FC0, 0x7E00), "nan-": (0xFFC00000, 0xFFC0, 0xFE00),
    "nan+payload": (0x7FC10000, 0x7FC1, 0x7E01), "nan-payload": (0xFFC10000, 0xFFC1, 0xFE01),
}
# (lower row, higher row) compete for one box: the order of the two decides who is the true positive
SCORE_PAIRS = [("nan-", "-inf"), ("-inf", "nan-"), ("nan+", "nan-"), ("nan-", "nan+"), ("nan+payload", "nan+"),
               ("nan-payload", "nan-"), ("+inf", "nan+"), ("nan-", "+inf"), ("-0", "+0"), ("+0", "-0"), ("2^-24", "+0"),
               ("2^-24", "2^-23"), ("-0.5", "-0"), ("-2^-24", "-0"), ("+inf", "1"), ("-inf", "-0.5"), ("nan-", "1")]
SCORE_TYPES = {"f32": (F32, 0, torch.int32), "bf16": (BF16, 1, torch.int16), "f16": (F16, 2, torch.int16)}


def score_tensor(kind, width):
    """[1, width] of the type from the bit patterns of SCORE_PAIRS, row 2 i and 2 i + 1 for pair i."""
    dtype, col, itype = SCORE_TYPES[kind]
    bits = [SCORE_BITS[n][col] for pair in SCORE_PAIRS for n in pair]
    bits = [b - (1 << (32 if col == 0 else 16)) if b >= 1 << (31 if col == 0 else 15) else b for b in bits]
    t = torch.zeros(1, width, dtype=itype)
    t[0, :len(bits)] = torch.tensor(bits, dtype=itype)
    return t.view(dtype)


def score_scene(kind):
    """One box per pair of SCORE_PAIRS, 5 m apart, and the pair's two predictions 0.125 and 0.25 m from it: whichever
    comes first in the order takes the box at every threshold, the other one is a false positive."""
    n = len(SCORE_PAIRS)
    raw = score_tensor(kind, 2 * n)
    gt = [TE.box(5.0 * (i % 8) - 17.5, 5.0 * (i // 8) - 5.0) for i in range(n)]
    preds = [TE.box(g[0] + 0.125 * (1 + k), g[1]) for g in gt for k in (0, 1)]
    # the scores the oracle sees: the exact widening of the type's bit patterns, made here (a host conversion need not
    # keep a NaN's sign or payload)
    col = SCORE_TYPES[kind][1]
    bits = np.array([SCORE_BITS[k][col] for pair in SCORE_PAIRS for k in pair], dtype=np.uint32)
    if kind == "f16":                     # 0x7e01 widens to 0x7fc02000: exponent 0xff, the ten mantissa bits on top
        mag, sign = bits & 0x7fff, (bits & 0x8000) << 16
        wide16 = bits.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32)
        bits = np.where(mag > 0x7c00, sign | 0x7f800000 | ((mag & 0x3ff) << 13), wide16)
    elif kind == "bf16":
        bits = bits << 16
    wide = bits.astype(np.uint32).view(np.float32)
    s = TE.sample(preds, wide, [CAR] * (2 * n), gt, [CAR] * n)
    return s, raw


@functools.lru_cache(maxsize=None)
def ev_case(name):
    """(samples, width, run_case keywords) of a detection-scoring case."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("gt"):
        n = int(name[2:])
        return [TE.random_scene(rng, n, 24, [PED], spread=20.0, on_ranges=False)], 24, {}
    if name.startswith("G"):
        return [interleaved(int(name[1:]), 40, int(name[1:]))], 40, {}
    if name == "M2048":
        s = TE.random_scene(rng, 30, 2048, [CAR], spread=25.0, score_levels=64, on_ranges=False)
        s["labels"][rng.permutation(2048)[:148]] = PED
        return [s], 2048, dict(protocol=BIG)
    if name == "M513":
        return [TE.random_scene(rng, 30, 513, [CAR, PED], spread=30.0, score_levels=64)], 513, dict(protocol=BIG)
    if name == "classes16":
        return [TE.random_scene(rng, 40, 48, list(range(16)), score_levels=6) for _ in range(2)], 48, dict(names=NAMES16)
    if name.startswith("tie"):
        return [tie_scene(name == "tie-registers")], 8, {}
    if name == "nonfinite-centres":
        s = nonfinite_scene()
        return [s], len(s["labels"]), {}
    kind = name.split("-")[1]
    s, raw = score_scene(kind)
    return [s], raw.shape[1], dict(score_dtype=SCORE_TYPES[kind][0], raw_scores=raw)


EV_CASES = ([f"gt{n}" for n in GT_SIZES] + ["G600", "G1100", "M2048", "M513", "classes16", "tie-lanes", "tie-registers",
                                             "nonfinite-centres"] + [f"scores-{k}" for k in SCORE_TYPES])


@gpu
@pytest.mark.parametrize("name", EV_CASES)
def test_det_eval_paths(dev, name):
    """Records, npos and scores against o_match / o_scores through test_det_eval.run_case."""
    samples, width, kw = ev_case(name)
    ev, matched = TE.run_case(samples, dev, width, **kw)
    names = kw.get("names", TE.NAMES)
    npred = [len(m["preds"]) for m in matched]
    tps = sorted({p[3] for m in matched for p in m["preds"]})
    print(f"[det_eval:{name}] npos {[m['npos'] for m in matched]}, predictions kept {npred}, true-positive bit sets {tps}")
    assert len(matched) == len(names) and sum(p[3] != 0 for m in matched for p in m["preds"]) > 0
    if name.startswith("tie"):
        # at each place both predictions match from the place's threshold on; at the first three, whose match is
        # recorded at the 2 m true-positive threshold, the scale error shows that the better prediction took the LOWER
        # row (1 x 1 x 1: 1 - 1 / 12) and the other one the higher; at the fourth (first matched at 4 m) no error is
        # recorded and the records say only that both matched
        preds = {p[2]: p for p in matched[PED]["preds"]}
        for j in range(4):
            first, second = preds[2 * j], preds[2 * j + 1]
            assert first[3] == second[3] == (0b1111 << j) & 0b1111, (j, first[3], second[3])
            if j <= 2:
                assert np.float32(first[4]["scale_err"]) == np.float32(1 - 1 / 12) and second[4]["scale_err"] == 0.0, j
    if name == "nonfinite-centres":
        assert matched[CAR]["npos"] == 6 and npred[CAR] == 6 and all(p[3] == 0b1111 for p in matched[CAR]["preds"])
    if name.startswith("scores"):
        order = [p[2] for p in matched[CAR]["preds"]]
        rows = TE.record_rows(ev, 1)
        for i, pair in enumerate(SCORE_PAIRS):
            first = min((2 * i, 2 * i + 1), key=order.index)
            assert (int(rows[first, 1]) >> 16, int(rows[first ^ 1, 1]) >> 16) == (0b1111, 0), (pair, first)


# =====================================================================================================================
# CPU tests: what the cases reach, the mirrors against the library
# =====================================================================================================================
def test_confusion_cases_reach_every_regime():
    reached = set()
    for name, c in CONF_CASES.items():
        mode = conf_mode(c.layout, c.S, c.misaligned)
        V = 4 if mode == "planes4" else 1
        lo, hi = c.window or (0, c.K)
        assert conf_valid(c.B, c.S, c.K, 0, _capi.VAMP_F32, T_CODE[c.tdtype], c.kc, lo, hi), name
        trips, last = conf_trips(c.n, V)
        grid = conf_grid(c.n, V)
        nb, reread = conf_batches(lo, hi)
        tname = str(c.tdtype)[6:]
        reached |= {f"{mode}-trips{trips}", f"{mode}-{tname}-mask{int(c.mask)}" + ("" if trips == 1 else f"-trips{trips}"),
                    f"batches{nb}-reread{reread}"}
        reached |= {k for k, v in (("one-trip-exactly", trips == 1 and c.n // V == CONF_STRIDE),
                                   ("second-trip-one-lane-group", trips == 2 and last == 1),
                                   (f"{mode}-third-trip-one-lane-group", trips == 3 and last == 1),
                                   ("slabs1024", grid == CONF_MAX_GRID), ("Kc32-bins1025-reduce17", c.kc == 32 and cdiv(c.kc ** 2 + 1, 64) == 17),
                                   ("Kc1", c.kc == 1), ("two-calls", c.calls == 2),
                                   (f"misaligned-{c.misaligned}-falls-back", c.misaligned and c.S % 4 == 0 and mode == "planes"),
                                   (f"window-w{hi - lo}-inside", c.window and lo > 0 and hi < c.K),
                                   (f"{mode}-ignore", c.ignore is not None)) if v}
        if trips > 1:
            live = conf_live_groups(name)
            pad = torch.zeros(trips * CONF_STRIDE, dtype=torch.bool)
            pad[:len(live)] = live
            exists = torch.arange(trips * CONF_STRIDE) < len(live)
            w_live = pad.view(trips, -1, 64).any(2)
            w_full = exists.view(trips, -1, 64).all(2)                # every lane of the wave has a group in that trip
            how = {h for _, _, h in c.dead}
            for k in range(trips - 1):
                if bool((~w_live[k] & w_full[k] & w_live[k + 1]).any()):
                    reached |= {f"wave-dead-then-live-by-{h}" for h in how}
                if bool((w_live[k] & ~w_live[k + 1] & w_full[k + 1]).any()):
                    reached |= {f"wave-live-then-dead-by-{h}" for h in how}
                if bool((w_live[k] & ~exists.view(trips, -1, 64).any(2)[k + 1]).any()):
                    reached.add("wave-live-then-past-the-end")
        if c.window:
            x, _, m = conf_inputs(name)[0]
            rows = x.reshape(-1, c.K)
            if reread and bool(rows[:, hi - 1].isnan().any()):
                reached.add(f"nan-on-the-reread-class-w{hi - lo}")
            if reread and bool((rows[:, lo:hi] == float("-inf")).all(1).any()):
                reached.add(f"all-minus-inf-window-reread-w{hi - lo}")
    required = ({"rows-trips1", "rows-trips2", "rows-trips3", "planes4-trips2", "planes-trips1", "planes4-trips1",
                 "one-trip-exactly", "second-trip-one-lane-group", "rows-third-trip-one-lane-group", "slabs1024",
                 "Kc32-bins1025-reduce17", "Kc1", "two-calls", "wave-dead-then-live-by-mask", "wave-live-then-dead-by-mask",
                 "wave-dead-then-live-by-ignore", "wave-live-then-past-the-end", "planes4-ignore", "rows-ignore",
                 "nan-on-the-reread-class-w10", "all-minus-inf-window-reread-w19", "batches1-reread8", "batches1-reread0",
                 "batches2-reread0", "batches3-reread0", "batches3-reread8"}
                | {f"window-w{w}-inside" for w in (1, 8, 9, 10, 18, 19, 27)}
                | {f"planes4-{t}-mask{m}" for t in ("int64", "int32", "uint8") for m in (0, 1)}
                | {f"misaligned-{w}-falls-back" for w in ("pred", "target", "mask")})
    assert not _unreached(required, reached), f"confusion regimes no case reaches: {_unreached(required, reached)}"
    # what test_seg_metrics runs: two samples of the occupancy grid take a second trip in the 4-wide mode (one sample
    # stays at 160 000 lane groups); the rows mode and the one-element planes mode never leave the first
    assert conf_trips(200 * 200 * 16, 4) == (1, 160000) and conf_trips(2 * 200 * 200 * 16, 4) == (2, 320000 - CONF_STRIDE)
    assert conf_trips(35011, 1)[0] == 1 and conf_trips(2 * 40 * 40 * 16, 1)[0] == 1
    assert conf_trips(CONF_STRIDE, 1) == (1, CONF_STRIDE) and conf_trips(CONF_STRIDE + 1, 1) == (2, 1)
    assert conf_trips(2 * CONF_STRIDE + 1, 1) == (3, 1) and conf_trips(4 * CONF_STRIDE + 4, 4) == (2, 1)


def test_lidarseg_cases_reach_every_regime():
    reached = set()
    for name, c in LS_CASES.items():
        logits, idx = ls_inputs(name)
        assert ls_workspace(c.P, c.R) > 0 and c.window[1] - c.window[0] <= 64 and logits.dtype == c.dtype, name
        keep = (idx >= 0) & (idx < c.R)
        runs = torch.bincount(idx[keep], minlength=c.R) if bool(keep.any()) else torch.zeros(c.R, dtype=torch.int64)
        reached |= {f"R{c.R}", f"tiles{ls_tiles(c.R)}", f"window{c.window[1] - c.window[0]}", str(c.dtype)[6:]}
        reached |= {k for k, v in (("R+1-fills-a-tile", (c.R + 1) % SCAN_TILE == 0), ("R+1-one-past-a-tile", (c.R + 1) % SCAN_TILE == 1),
                                   ("run>256-between-empty-runs", c.scene == "long-run" and int(runs[LS_LONG[0]]) > 256
                                    and int(runs[LS_LONG[0] - 1]) == 0 == int(runs[LS_LONG[0] + 1])),
                                   ("every-index-out-of-range", c.P > 0 and not bool(keep.any())),
                                   ("negative-and-beyond", bool((idx < 0).any()) and bool((idx >= c.R).any()))) if v}
    required = {"R2047", "R2048", "R2049", "R4097", "tiles1", "tiles2", "tiles3", "R+1-fills-a-tile", "R+1-one-past-a-tile",
                "window64", "window1", "window16", "run>256-between-empty-runs", "every-index-out-of-range",
                "negative-and-beyond", "bfloat16", "float32"}
    assert not _unreached(required, reached), f"lidar-seg regimes no case reaches: {_unreached(required, reached)}"
    assert ls_tiles(3500) == 2 and ls_tiles(600) == 1                  # what test_seg_metrics runs


def test_camera_image_cases_reach_every_regime():
    reached = set()
    for name, c in IMG_CASES.items():
        plan = img_plan(name)
        H, W = c.final
        tx, ty = img_taps(plan)
        crops = [t[2] for t in img_augs(c)[0]]
        new_w, new_h = img_augs(c)[0][0][1]
        assert img_lds(plan.foot_w, plan.foot_h) + 4 * (IMG_K * IMG_TW + IMG_TH * IMG_K + 4 * 64 + 4) <= 64 * 1024, name
        reached |= {f"W{W}", f"H{H}", f"tiles{cdiv(H, IMG_TH)}x{cdiv(W, IMG_TW)}", f"taps{max(tx, ty)}",
                    {F32: "fp32", BF16: "bf16", None: "u8-alone"}[c.dtype] + ("-vector" if W % 4 == 0 else "-element")}
        reached |= {k for k, v in (("foot_w>160", plan.foot_w > 160), ("foot_h>30", plan.foot_h > 30),
                                   ("upscale2", c.resize == 2.0), ("upscale3", c.resize == 3.0),
                                   ("whole-column-tiles", W % IMG_TW == 0), ("whole-row-tiles", H % IMG_TH == 0),
                                   ("overrun-left-and-bottom", any(x0 < 0 and y1 > new_h for x0, _, _, y1 in crops)),
                                   ("overrun-right-and-top", any(x1 > new_w and y0 < 0 for _, y0, x1, _ in crops)),
                                   ("flips-and-rotations", {(t[3], t[4]) for t in img_augs(c)[0]}
                                    == set(itertools.product((False, True), TI.ROTATES))),
                                   ("to_rgb0", not c.to_rgb),
                                   ("four-row-phases", {(3 + r * img_row_stride(c)) % 4 for r in range(c.raw_hw[0])} == {0, 1, 2, 3}
                                    and c.pad_w > 0)) if v}
        if c.raw_hw == CORNER_RAW:
            reached.add(f"resize{c.resize}-{H}x{W}-pitch{img_raw_pitch(plan.foot_w)}")
    required = ({f"W{w}" for w in (1, 3, 5, 44, 64, 70, 128)} | {f"H{h}" for h in (1, 7, 8, 9, 16, 18, 20)}
                | {"taps15", "taps16", "foot_w>160", "foot_h>30", "upscale2", "upscale3", "whole-column-tiles", "whole-row-tiles",
                   "tiles2x2", "tiles3x2", "tiles3x1", "bf16-element", "u8-alone-element", "fp32-vector", "fp32-element",
                   "overrun-left-and-bottom", "overrun-right-and-top", "flips-and-rotations", "to_rgb0", "four-row-phases",
                   "resize0.254-18x70-pitch804", "resize0.254-20x44-pitch564", "resize0.27-18x70-pitch756"})
    assert not _unreached(required, reached), f"image regimes no case reaches: {_unreached(required, reached)}"
    # the corner: 0.254 is the smallest resize (to 0.001) the plan accepts for this raw size; it needs every tap the
    # library holds, and no accepted resize needs a wider or taller footprint.  0.27 gives 15 taps and 41 x 250.
    plan = img_plan("corner-18x70")
    assert img_taps(plan) == (IMG_K, IMG_K) and (plan.foot_h, plan.foot_w) == (44, 265)
    p27 = img_plan("resize0.27-18x70")
    assert img_taps(p27) == (15, 15) and (p27.foot_h, p27.foot_w) == (41, 250)
    c = IMG_CASES["corner-18x70"]
    for r in (0.25, CORNER_RESIZE - 0.001):
        with pytest.raises(ValueError, match="outside its range"):
            I.plan_camera_images(img_augs(dataclasses.replace(c, resize=r)), c.raw_hw, c.final)
    for r in np.arange(CORNER_RESIZE, 1.31, 0.004):
        p = I.plan_camera_images(img_augs(dataclasses.replace(c, resize=float(r))), c.raw_hw, c.final)
        assert max(img_taps(p)) <= IMG_K and p.foot_w <= plan.foot_w and p.foot_h <= plan.foot_h, r
    # what test_camera_images runs: raw rows of at most 160 pixels
    assert I.plan_camera_images(TI.sweep_augs((90, 160), (18, 70)), (90, 160), (18, 70)).foot_w <= 160


def test_point_query_cases_reach_every_regime():
    reached = set()
    for name, c in PQ_CASES.items():
        case = pq_case(c)
        pts, counts, occ, (s_union, s_big) = pq_scene(name)
        assert pq_workspace(3, c.K, c.Z, c.Y, c.X, pts.shape[1], occ.shape[1]) > 0, name
        cp, cp4, pad = pq_cp(c.K)
        n = pq_union_records(name)
        heavy, light = int((n > PQ_HEAVY).sum()), int(((n > 0) & (n <= PQ_HEAVY)).sum())
        at = lambda s: int(n[0, s[2], s[1], s[0]])
        parts = "".join(k for k, v in zip("LSO", (c.lidar, c.lidar and c.sdf, c.occupancy)) if v)
        if heavy and light:
            reached.add(f"CP4={cp4}-pad{pad}-gather-and-heavy")
        reached |= {f"runs_x{cdiv(c.X, PQ_PVPB)}-X{c.X}", f"Y{c.Y}", f"Z{c.Z}", f"parts-{parts}-{c.mode}", str(c.den_dtype)[6:]}
        reached |= {k for k, v in (("shared-grid", c.shared), ("upstream-for-some", not all(c.given)),
                                   ("count-0-between-live", counts[1] == 0 and counts[0] > 0 and counts[2] > 0),
                                   ("count-0-last", counts[2] == 0),
                                   ("heavy-through-the-union-alone", c.lidar and c.occupancy and at(s_union) > PQ_HEAVY),
                                   ("heavy-by-lidar-alone", c.lidar and at(s_big) > PQ_HEAVY)) if v}
        if c.lidar:
            assert at(s_big) >= 600, name
    required = ({f"CP4={k}-pad{p}-gather-and-heavy" for k, p in ((1, 2), (2, 3), (3, 3), (4, 3), (6, 3), (7, 3), (2, 0), (3, 0), (4, 0), (1, 0))}
                | {"runs_x1-X5", "runs_x1-X32", "runs_x2-X33", "runs_x3-X65", "Y1", "Z1", "parts-LSO-sdf", "parts-O-sdf", "parts-LS-sdf",
                   "parts-LO-sdf", "parts-LO-naive", "bfloat16", "float32", "shared-grid", "upstream-for-some",
                   "count-0-between-live", "count-0-last", "heavy-through-the-union-alone", "heavy-by-lidar-alone"})
    assert not _unreached(required, reached), f"point-query regimes no case reaches: {_unreached(required, reached)}"
    assert [pq_cp(k)[1] for k in (3, 18, 31)] == [1, 5, 8]             # what test_gradients_against_float64 runs


def test_det_eval_cases_reach_every_regime():
    reached = set()
    for name in EV_CASES:
        samples, width, kw = ev_case(name)
        names = kw.get("names", TE.NAMES)
        G = max(len(s["gt_labels"]) for s in samples)
        reached |= {f"G-trips{cdiv(G, EV_BLOCK)}", f"M-trips{cdiv(width, EV_BLOCK)}", f"classes{len(names)}"}
        for c in range(len(names)):
            for ngt, npred in survivors(samples, c, names):
                assert ngt <= EV_GT_CAP, name
                if npred:
                    reached.add(f"act{ev_act(ngt)}")
                    if name.startswith("gt"):
                        reached.add(f"gt{ngt}-act{ev_act(ngt)}{'-ragged' if ngt % EV_PER_LANE else ''}")
                    if npred > 1800:
                        reached.add("predictions>1800-of-one-class")
        if name.startswith("G"):
            lab = samples[0]["gt_labels"]
            ped = np.nonzero(lab == PED)[0]
            if bool((lab == -1).any()) and len(set(lab.tolist())) >= 6 and len(set(ped // EV_BLOCK)) == cdiv(G, EV_BLOCK):
                reached.add(f"interleaved-G{G}")
        if name.startswith("tie"):
            m = TE.o_match(samples)[PED]["preds"]
            reached |= {f"{name}-first-hit-at-threshold{h}" for h in range(4) if any(p[3] == (0b1111 << h) & 0b1111 for p in m)}
        if name == "nonfinite-centres":
            s = samples[0]
            for what, b in (("pred", s["boxes"]), ("gt", s["gt_boxes"])):
                reached |= {f"{what}-centre-{k}" for k, v in (("nan", np.isnan(b[:, :2]).any()), ("+inf", (b[:, :2] == np.inf).any()),
                                                              ("-inf", (b[:, :2] == -np.inf).any())) if v}
        if name.startswith("scores"):
            kind = name.split("-")[1]
            raw = kw["raw_scores"]
            v = raw.float()[0].numpy()
            sign = np.signbit(v)
            reached |= {f"{kind}-{k}" for k, ok in (("negative", (v < 0).any()), ("-0", ((v == 0) & sign).any()),
                                                    ("+0-beside", ((v == 0) & ~sign).any()), ("+inf", (v == np.inf).any()),
                                                    ("-inf", (v == -np.inf).any()), ("nan+", (np.isnan(v) & ~sign).any()),
                                                    ("nan-", (np.isnan(v) & sign).any()),
                                                    ("f16-subnormal-value", ((np.abs(v) > 0) & (np.abs(v) < 2.0 ** -14)).any())) if ok}
            assert raw.dtype == SCORE_TYPES[kind][0]
    required = ({f"gt{n}-act{ev_act(n)}{'-ragged' if n % 4 else ''}" for n in GT_SIZES} | {f"act{a}" for a in (1, 2, 4, 8, 16, 32, 64)}
                | {"G-trips1", "G-trips3", "G-trips5", "M-trips1", "M-trips3", "M-trips8", "classes10", "classes16",
                   "interleaved-G600", "interleaved-G1100", "predictions>1800-of-one-class"}
                | {f"tie-{w}-first-hit-at-threshold{h}" for w in ("lanes", "registers") for h in range(4)}
                | {f"{w}-centre-{k}" for w in ("pred", "gt") for k in ("nan", "+inf", "-inf")}
                | {f"{t}-{k}" for t in SCORE_TYPES for k in ("negative", "-0", "+0-beside", "+inf", "-inf", "nan+", "nan-",
                                                             "f16-subnormal-value")})
    assert not _unreached(required, reached), f"det_eval regimes no case reaches: {_unreached(required, reached)}"
    assert [ev_act(n) for n in (1, 4, 5, 63, 64, 65, 128, 129, 256)] == [1, 1, 2, 16, 16, 32, 32, 64, 64]
    assert {ev_act(min(n, EV_GT_CAP)) for n in (1, 63, 64, 65, 66, 67, 68, 256, 257, 258, 259)} == {1, 16, 32, 64}   # test_det_eval's


def test_tie_scenes_are_ties_in_the_oracle():
    """The two boxes of a place are equally far from both predictions (exactly, in float64), the distance lies between
    two thresholds, and the oracle gives the lower row to the better prediction."""
    for same_lane in (False, True):
        s = tie_scene(same_lane)
        for j, d in enumerate((0.25, 0.75, 1.5, 3.0)):
            lo, hi = (2 * j, 2 * j + 1) if same_lane else (j, j + 4)
            assert lo // EV_PER_LANE == hi // EV_PER_LANE if same_lane else lo // EV_PER_LANE != hi // EV_PER_LANE
            for r in (2 * j, 2 * j + 1):
                d2 = [float((s["gt_boxes"][g, 0] - s["boxes"][r, 0]) ** 2 + (s["gt_boxes"][g, 1] - s["boxes"][r, 1]) ** 2) for g in (lo, hi)]
                assert d2[0] == d2[1] == d * d and (TE.THS[j - 1] if j else 0.0) < d < TE.THS[j]
        m = {p[2]: p for p in TE.o_match([s])[PED]["preds"]}
        assert all(m[2 * j][4] is None or m[2 * j][4]["scale_err"] > 0.9 for j in range(4))


def test_oracle_orders_nan_scores_above_every_number():
    """The rule of vamp_det_eval_update's header in the oracle: a NaN of either sign first, NaNs equal among themselves
    (higher row first), -0.0 equal to +0.0."""
    nan = float("nan")
    gt = ([TE.box(0, 0)], [CAR])
    order = lambda scores: [p[2] for p in TE.o_match([TE.sample([TE.box(0.25, 0)] * len(scores), scores, [CAR] * len(scores), *gt)])[CAR]["preds"]]
    assert order([1.0, -nan, float("inf"), nan, 0.5]) == [3, 1, 2, 0, 4]
    assert order([-nan, float("-inf")]) == [0, 1] and order([nan, -nan]) == [1, 0] and order([-0.0, 0.0, -0.0]) == [2, 1, 0]
    s, raw = score_scene("bf16")
    assert np.signbit(s["scores"][np.isnan(s["scores"])]).any() and raw.dtype == BF16


def test_host_score_keys_order_like_the_oracle():
    """metrics._score_keys, which the epoch-end sort of the records uses, against the oracle's order on the score
    scene: slots descending, then a stable descending sort by key, is the oracle's order."""
    for kind in SCORE_TYPES:
        s, _ = score_scene(kind)
        want = [p[2] for p in TE.o_match([s])[CAR]["preds"]]
        idx = torch.arange(len(s["scores"])).flip(0)
        keys = metrics._score_keys(torch.from_numpy(s["scores"].view(np.int32).copy()))[idx]
        assert idx[torch.sort(keys, stable=True, descending=True).indices].tolist() == want, kind


# ----------------------------------------------------------------------------------- the mirrors against the library
@pytest.fixture(scope="module")
def lib():
    from vampire_amd.build import build_library
    build_library(verbose=False)
    return _capi.load()


def test_confusion_and_lidarseg_host_answers_match_the_mirror(lib):
    sizes = [(1, 0), (1, 1), (1, 255), (1, 256), (1, 257), (1, CONF_STRIDE - 1), (1, CONF_STRIDE), (1, CONF_STRIDE + 1),
             (2, 200 * 200 * 16), (7, 1 << 28), (1, I31 - 1), (1, I31), (1 << 16, 1 << 15), (1 << 16, (1 << 15) - 1), (-1, 5)]
    n = 0
    for (B, S), (K, Kc, lo, hi), layout, pdt, tdt in itertools.product(
            sizes, ((18, 18, 0, 18), (18, 17, 1, 17), (32, 32, 0, 32), (1, 1, 0, 1), (30, 29, 2, 29), (33, 33, 0, 33), (18, 17, 0, 18),
                    (18, 0, 0, 18), (18, 18, 5, 5), (1, 6, 0, 1)),
            (_capi.VAMP_SEG_ROWS, _capi.VAMP_SEG_PLANES, 2), (_capi.VAMP_F32, _capi.VAMP_BF16, _capi.VAMP_I64, _capi.VAMP_F16),
            (_capi.VAMP_I64, _capi.VAMP_U8, _capi.VAMP_F32)):
        d = TM._desc(B=B, S=S, K=K, layout=layout, pred_dtype=pdt, target_dtype=tdt, Kc=Kc, lo=lo, hi=hi)
        want = conf_workspace(B, S, K, layout, pdt, tdt, Kc, lo, hi)
        assert lib.vamp_confusion_workspace_bytes(C.byref(d)) == want, (B, S, K, Kc, lo, hi, layout, pdt, tdt)
        n += want > 0
    assert n > 300 and conf_workspace(7, 1 << 28, 32, 0, _capi.VAMP_F32, _capi.VAMP_I64, 32, 0, 32) == 1024 * 1025 * 4
    for name, c in CONF_CASES.items():
        lo, hi = c.window or (0, c.K)
        d = TM._desc(B=c.B, S=c.S, K=c.K, layout=int(c.layout == "planes"), target_dtype=T_CODE[c.tdtype], Kc=c.kc, lo=lo, hi=hi)
        assert lib.vamp_confusion_workspace_bytes(C.byref(d)) == conf_grid(c.n, 1) * (c.kc ** 2 + 1) * 4 > 0, name
    for P, R in itertools.product((0, 1, 3000, 1 << 20, I31 - 1, I31, -1), (0, 1, 2046, 2047, 2048, 2049, 4097, 1 << 24,
                                                                            I31 - 2 * SCAN_TILE - 1, I31 - 2 * SCAN_TILE, -1)):
        assert lib.vamp_lidarseg_workspace_bytes(P, R) == ls_workspace(P, R), (P, R)
    assert ls_workspace(I31 - 1, 1 << 24) > 1 << 34


def test_camera_images_host_answers_match_the_mirror(lib):
    n = 0
    for B, N, H, W, foot_w, foot_h, dt in itertools.product((0, 1, 5, 4096, 4097), (1, 6, 16, 17), (1, 7, 8, 9, 900, 4096, 4097),
                                                            (1, 3, 5, 64, 70, 1600, 4096), (1, 160, 250, 272, 273), (1, 41, 48, 49),
                                                            (_capi.VAMP_F32, _capi.VAMP_BF16, _capi.VAMP_IMG_OUT_NONE, _capi.VAMP_F16)):
        d = TI._desc(B=B, N=N, H=H, W=W, foot_w=foot_w, foot_h=foot_h, out_dtype=dt)
        assert lib.vamp_camera_images_workspace_bytes(C.byref(d)) == img_workspace(d), (B, N, H, W, foot_w, foot_h, dt)
        n += img_valid(d)
    assert n > 1000 and img_workspace(TI._desc(B=4095, N=16, H=4096, W=4096)) > 1 << 41
    assert img_raw_pitch(272) == 820 and img_raw_pitch(250) == 756 and img_raw_pitch(1) == 12 and img_lds(272, 48) == 48 * 1012
    assert all((img_raw_pitch(w) // 4) % 2 == 1 and img_raw_pitch(w) >= 3 * w + 3 for w in range(1, 273))


def test_point_queries_host_answers_match_the_mirror(lib):
    n = 0
    for K, X, Y, Z, B, M, P in itertools.product((0, 1, 3, 4, 7, 8, 24, 31, 32), (1, 5, 32, 33, 65, 2046, 2047), (1, 16, 2046),
                                                 (1, 5, 510, 511), (1, 3), (0, 63, 1 << 20), (0, 385, 200 * 200 * 16)):
        d = TQ.query_desc(K=K, X=X, Y=Y, Z=Z, B=B, M=M, P=P)
        d.K = K
        want = pq_workspace(B, K, Z, Y, X, M, P)
        assert lib.vamp_point_queries_workspace_bytes(C.byref(d)) == want, (K, X, Y, Z, B, M, P)
        n += want > 0
    assert n > 1000 and pq_workspace(3, 31, 510, 2046, 2046, 1 << 20, 200 * 200 * 16) == 0       # voxels beyond 2^31
    assert pq_workspace(3, 31, 5, 2046, 2046, 1 << 20, 200 * 200 * 16) > 1 << 30
    assert [pq_cp(k) for k in (1, 3, 4, 7, 8, 31)] == [(4, 1, 2), (4, 1, 0), (8, 2, 3), (8, 2, 0), (12, 3, 3), (32, 8, 0)]


def test_det_eval_host_answers_match_the_mirror(lib):
    n = 0
    for B, M, G, ncls, ms, mb in itertools.product((0, 1, 2, 4096, 4097), (0, 1, 513, 2048, 2049), (-1, 0, 600, 1 << 20, (1 << 20) + 1),
                                                   (0, 1, 10, 16, 17), (0, 1, 8, 1 << 20, (1 << 20) + 1, 1 << 30), (0, 1, 500, 2048)):
        d = TE._desc(B=B, M=M, G=G, num_classes=min(ncls, 16) if ncls != 17 else 17, max_samples=ms, max_boxes_per_sample=mb)
        if d.num_classes > 10:          # (the defaults carry ten classes' ranges: the others need one to be valid)
            for c in range(10, min(d.num_classes, 16)):
                d.class_range[c] = 50.0
        want = ev_record_bytes(d)
        assert lib.vamp_det_eval_record_bytes(C.byref(d)) == want, (B, M, G, ncls, ms, mb)
        assert lib.vamp_det_eval_supported(C.byref(d)) == int(want > 0)
        n += want > 0
    assert n > 300 and ev_record_bytes(TE._desc(M=2048, max_samples=(1 << 20) - 1)) > 1 << 35
