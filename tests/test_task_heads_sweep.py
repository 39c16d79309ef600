"""The task-head kernels across the sizes that pick their code paths -- seg_loss.hip, det_targets.hip, det_loss.hip,
det_post.hip and rgb_loss.hip -- with the oracles, input builders, comparison helpers and bars of the kernels' own test
modules (test_seg_loss, test_det_targets, test_det_loss, test_det_postprocess, test_rgb_loss), none of them restated
or loosened: every case here is a shape, a task table or a placement those modules do not run.

seg_loss     the histogram scan's turns of 16 384 counters (one full turn, a second turn of 256 counters, three turns),
             channel-first uint8 input in its second turn, whole 2048-record tiles masked out, a class without
             foreground, and the sort's exactness check on a two-turn case.
det_targets  classes 2 and 3 of a task (n2 / n3, run2 / run3, v2 / v3, pick4): task tables (3, 4, 1), (4,) and eight
             tasks of every class count, maps with partial tiles in both directions, box counts around the 256-box
             chunk with runs of class 2 and class 3 across a wave and across the chunk, truncation inside class 2 and
             class 3.  Bit-exact.
det_loss     class counts (4, 3, 1), eight tasks, B = 65 (the finish kernel's second turn), max_objs 255 / 256 / 257 /
             4096 with many live slots of one cell on both sides of the 256-slot chunk, with and without velocity.
det_post     class indices 2 and 3 in the decode, K = 1 / 63 / 64 / 65 / 128 below N, K = N < 64, 7 x 150, one task,
             eight tasks whose K differ, candidate counts 63 / 64 / 65 with suppression from the first 64-row block
             into the second, post_max_size reached in the second block, pre_max_size 1 / 63 / 65 under rotated NMS,
             and pairs of boxes of known closed-form IoU (identical, shifted, touching, contained flush, quarter- and
             half-turn copies, the 45-degree octagon) with the threshold 1e-3 (relative) either side of it.
rgb_loss     C = 2 and 4, N = 5, valid extents that are whole numbers of tiles, a strongly non-square image.

The CPU tests at the end mirror the host formulas that choose these paths, map every GPU case through them and fail
with the name of any listed regime that no case reaches; compare the mirrors with the library's *_workspace_bytes over
grids of descriptors that include sizes no GPU test could allocate; and check the crafted pairs against the float64
clip and their closed forms.

Measured on an MI355X: the 42 GPU tests of this file take 9 to 10 s in all; the slowest single case is rgb_loss (2, 4, 186,
202) at 4 s (the first rgb case of the run), and no other case takes more than 1.5 s."""
import ctypes as C
import dataclasses
import functools
import itertools
import math

import pytest
import torch

import test_det_loss as TL
import test_det_postprocess as TP
import test_det_targets as TT
import test_rgb_loss as TR
import test_seg_loss as TS
from vampire_amd import _capi, ops
from vampire_amd import multitask as M
from vampire_amd.config import CFG_A
from test_seg_loss import dev  # noqa: F401  (the module-scoped device fixture)

gpu = pytest.mark.gpu
I31 = 1 << 31


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cdiv(a, b):
    return -(-a // b)


def align_up(v, a):
    return cdiv(v, a) * a


# =====================================================================================================================
# mirrors of the host formulas
# =====================================================================================================================
# ------------------------------------------------------------------------------------------------ seg_loss.hip
SEG_TILE, SEG_RADIX, SEG_SCAN_TURN, SEG_BLOCK, SEG_HDR = 2048, 256, 1024 * 16, 256, 64 * 4
SEG_LABELS = (_capi.VAMP_I64, _capi.VAMP_I32, _capi.VAMP_U8)


def seg_tiles(P):
    return cdiv(P, SEG_TILE)


def seg_scan_turns(P):
    """Turns of seg_scan_kernel over the 256 T digit counters of a class, and the entries of its last turn."""
    n = SEG_RADIX * seg_tiles(P)
    return cdiv(n, SEG_SCAN_TURN), n - (cdiv(n, SEG_SCAN_TURN) - 1) * SEG_SCAN_TURN


def seg_valid(B, S, Cn, layout=_capi.VAMP_SEG_ROWS, label=_capi.VAMP_I64):
    return (layout in (_capi.VAMP_SEG_ROWS, _capi.VAMP_SEG_PLANES) and 2 <= Cn <= 32 and B >= 1 and S >= 1
            and B < I31 and S < I31 and B * S < I31 and B * S * Cn < I31 and label in SEG_LABELS)


def seg_workspace(B, S, Cn, **kw):
    if not seg_valid(B, S, Cn, **kw):
        return 0
    P = B * S
    rec, tiles, nrow = Cn * P, Cn * seg_tiles(P), cdiv(P, SEG_BLOCK)
    return sum(align_up(n, 256) for n in (rec * 4,) * 4 + (tiles * SEG_RADIX * 4, tiles * 4, nrow * 4, nrow * 8, tiles * 8))


def seg_kept(B, S, Cn, **kw):
    return align_up(align_up(SEG_HDR, 256) + Cn * B * S * 4, 256) if seg_valid(B, S, Cn, **kw) else 0


# ------------------------------------------------------------------------------------------------ det_post.hip
POST_MAX_K, POST_SEL_BLOCK, POST_ROW, POST_WORDS = 1024, 1024, 12, 16


@dataclasses.dataclass(frozen=True)
class PostPlan:
    N: tuple            # heatmap elements per task
    K: tuple            # candidates selected per task
    KS: tuple           # the bitonic sort's padded length
    chunk: tuple        # keys per lane of the gather
    KP: int             # candidate rows per (sample, task): the largest K, padded to 64
    nblk: int           # 64-row blocks of the suppression matrix
    nstride: int


def post_valid(B, H, W, ncls, max_num, post, pre=1, rotate=False):
    return (1 <= B <= 1 << 20 and 1 <= len(ncls) <= 8 and H >= 1 and W >= 1 and max_num >= 1 and 1 <= post <= max_num
            and (not rotate or pre >= 1) and all(1 <= n <= 4 for n in ncls)
            and all(n * H * W < I31 - 1 and min(max_num, n * H * W) <= POST_MAX_K for n in ncls))


def post_plan(H, W, ncls, max_num):
    N = tuple(n * H * W for n in ncls)
    K = tuple(min(max_num, n) for n in N)
    KP = align_up(max(K), 64)
    return PostPlan(N, K, tuple(1 << max(k - 1, 0).bit_length() for k in K), tuple(cdiv(n, POST_SEL_BLOCK) for n in N),
                    KP, KP // 64, align_up(max(N), 64))


def post_workspace(B, H, W, ncls, max_num, post, pre=1, rotate=False):
    if not post_valid(B, H, W, ncls, max_num, post, pre, rotate):
        return 0
    p, BT = post_plan(H, W, ncls, max_num), B * len(ncls)
    return sum(align_up(n, 256) for n in (BT * p.nstride * 4, BT * p.KP * POST_ROW * 4, BT * 4, BT * p.KP * POST_WORDS * 8,
                                          BT * post * 4, BT * 4))


# ------------------------------------------------------------------------------------------------ det_loss.hip
LOSS_CHUNK, LOSS_BLOCK, LOSS_MAX_OBJS, LOSS_MAX_CHUNKS = 2048, 256, 4096, 1 << 22


@dataclasses.dataclass(frozen=True)
class LossPlan:
    heat_chunks: tuple  # 2048-element chunks of each task's heatmaps
    zchunks: int        # chunks per task of the regression gradient maps
    slot_turns: int     # 256-slot turns of the compaction in grad_box_kernel
    heat_turns: tuple   # 64-partial turns of the finish kernel's lane-strided sum over a task's heat chunks
    box_turns: int      # ... and over its B box partials


def loss_plan(B, H, W, K, ncls, code):
    hc = tuple(cdiv(B * n * H * W, LOSS_CHUNK) for n in ncls)
    return LossPlan(hc, cdiv(B * code * H * W, LOSS_CHUNK), cdiv(K, LOSS_BLOCK), tuple(cdiv(c, 64) for c in hc), cdiv(B, 64))


def loss_valid(B, H, W, K, ncls, code, has_vel):
    if not (1 <= B <= 4096 and 1 <= len(ncls) <= 8 and 1 <= H <= 8192 and 1 <= W <= 8192 and all(1 <= n <= 4 for n in ncls)
            and code in (8, 10) and has_vel in (0, 1) and code == (10 if has_vel else 8) and 1 <= K <= LOSS_MAX_OBJS):
        return False
    p = loss_plan(B, H, W, K, ncls, code)
    return sum(p.heat_chunks) + len(ncls) * p.zchunks <= LOSS_MAX_CHUNKS


def loss_workspace(B, H, W, K, ncls, code, has_vel):
    if not loss_valid(B, H, W, K, ncls, code, has_vel):
        return 0
    return align_up((sum(loss_plan(B, H, W, K, ncls, code).heat_chunks) + len(ncls) * B) * 8, 256)


# ------------------------------------------------------------------------------------------------ det_targets.hip
TGT_TILE_W, TGT_TILE_H, TGT_BLOCK = 32, 8, 256


def tgt_grid(fh, fw):
    """(tiles along x, tiles along y, columns of the last tile, rows of the last tile)"""
    ntx, nty = cdiv(fw, TGT_TILE_W), cdiv(fh, TGT_TILE_H)
    return ntx, nty, fw - (ntx - 1) * TGT_TILE_W, fh - (nty - 1) * TGT_TILE_H


def tgt_valid(B, M_, ncls, cols, code, max_objs, fh, fw, label=_capi.VAMP_I64):
    return (1 <= B <= 4096 and 1 <= len(ncls) <= 8 and 0 <= M_ <= 1 << 20 and all(1 <= n <= 4 for n in ncls)
            and cols in (7, 9) and code == cols + 1 and 1 <= max_objs <= 8192 and 1 <= fh <= 8192 and 1 <= fw <= 8192
            and label in (_capi.VAMP_I32, _capi.VAMP_I64))


def tgt_workspace(B, M_, ncls, cols, code, max_objs, fh, fw, **kw):
    if not tgt_valid(B, M_, ncls, cols, code, max_objs, fh, fw, **kw):
        return 0
    return align_up(B * len(ncls) * max_objs * 16, 256) + align_up(B * len(ncls) * 4, 256)


# ------------------------------------------------------------------------------------------------ rgb_loss.hip
RGB_SCALES, RGB_REACH, RGB_TW, RGB_TH, RGB_MIN, RGB_MAX = 5, 10, 32, 16, 176, 16384


@dataclasses.dataclass(frozen=True)
class RgbScale:
    H: int
    W: int
    tx: int             # tiles of the valid region
    ty: int
    lcols: int          # columns / rows the last tile of a row / column owns (its own and those behind the valid region)
    lrows: int


def rgb_scales(H, W):
    out = []
    for _ in range(RGB_SCALES):
        tx, ty = cdiv(W - RGB_REACH, RGB_TW), cdiv(H - RGB_REACH, RGB_TH)
        out.append(RgbScale(H, W, tx, ty, W - (tx - 1) * RGB_TW, H - (ty - 1) * RGB_TH))
        H, W = H // 2, W // 2
    return out


def rgb_valid(N, Cn, H, W):
    return N >= 1 and 1 <= Cn <= 4 and RGB_MIN <= H <= RGB_MAX and RGB_MIN <= W <= RGB_MAX and N * Cn * H * W < I31


def rgb_workspace(N, Cn, H, W):
    if not rgb_valid(N, Cn, H, W):
        return 0
    P, sc = N * Cn, rgb_scales(H, W)
    npart = sum(P * s.tx * s.ty for s in sc) + P * sc[0].tx * sc[0].ty
    nadj = sum(3 * P * (s.H - RGB_REACH) * (s.W - RGB_REACH) for s in sc)
    ng = sum(P * s.H * s.W for s in sc[1:])
    return sum(align_up(n, 256)
               for n in (npart * 8, N * RGB_SCALES * 8, N * RGB_SCALES * 8, N * 8, 2 * ng * 4, nadj * 4, ng * 4))


# =====================================================================================================================
# the case tables (all inputs are seeded CPU tensors: the CPU tests below read the same tables)
# =====================================================================================================================
# ---- seg_loss: rows layout, test_seg_loss.make_case as it stands: name -> (P, C)
SEG_ROWS_CASES = {"one-full-turn": (131072, 2), "second-turn-256": (131073, 2), "three-turns": (262145, 2)}
SEG_SORT_CASE = "second-turn-256"
SEG_PLANES = dict(B=3, S=43691, Cn=3)                               # B S = 131 073, S odd, uint8 labels, [B, C, S] memory
SEG_CLEARED = dict(P=136001, Cn=3, tiles=(0, 1, 31, 63, 64, 65))    # 67 tiles; the masked-out tiles, both sides of turn 2


@functools.lru_cache(maxsize=None)
def seg_planes_inputs():
    c = SEG_PLANES
    return TS.make_case(c["B"] * c["S"], c["Cn"], seed=7, label_dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def seg_cleared_inputs():
    """make_case, then labels over classes 0 and 1 only (class 2 has no foreground: G = 0) and whole tiles masked out."""
    c = SEG_CLEARED
    logits, labels, mask = TS.make_case(c["P"], c["Cn"], seed=8)
    labels = torch.where((labels >= 0) & (labels < c["Cn"]), torch.randint(0, 2, labels.shape, generator=gen(81)), labels)
    mask = mask.clone()
    for t in c["tiles"]:
        mask[t * SEG_TILE:(t + 1) * SEG_TILE] = False
    return logits, labels, mask


# ---- det_targets: name -> TgtCase
@dataclasses.dataclass(frozen=True)
class TgtCase:
    ncls: tuple
    fh: int
    fw: int
    M: int
    max_objs: int
    cols: int
    label_dtype: torch.dtype
    norm_bbox: bool = True
    B: int = 2


T8_NCLS = (1, 2, 3, 4, 4, 3, 2, 1)
TGT_CASES = {
    "t341-5x33-M255": TgtCase((3, 4, 1), 5, 33, 255, 100, 9, torch.int64),
    "t4-9x31-M256": TgtCase((4,), 9, 31, 256, 150, 7, torch.int32),
    "t4-40x7-M257": TgtCase((4,), 40, 7, 257, 300, 9, torch.int32, norm_bbox=False),
    "t8-9x31-M257": TgtCase(T8_NCLS, 9, 31, 257, 45, 7, torch.int64),
}


def tgt_cfg(c):
    tc = TT.train_cfg(CFG_A, grid_size=[c.fw * 4, c.fh * 4, 1], max_objs=c.max_objs)
    if c.cols == 7:
        tc["code_weights"] = tc["code_weights"][:8]
    return tc


@functools.lru_cache(maxsize=None)
def tgt_scene(name):
    """test_det_targets.random_scene's boxes (sizes, yaw, velocity), their centres spread over the case's map and a
    margin around it; labels over every class of the table and the two foreign values either side.  Sample 0 holds a
    run of class 3 of the last four-class task across the wave boundary at box 192 and one over the last boxes (across
    the 256-box chunk when M = 257); sample 1 the same runs of class 2."""
    c = TGT_CASES[name]
    tc = tgt_cfg(c)
    boxes, labels = TT.random_scene(c.B, c.M, CFG_A, 1000 + c.M, cols=c.cols, label_dtype=c.label_dtype)
    g = gen(2000 + c.M + c.fw)
    cell = tc["voxel_size"][0] * tc["out_size_factor"]
    pc0, pc1 = tc["point_cloud_range"][:2]
    total = sum(c.ncls)
    t4 = max(t for t, n in enumerate(c.ncls) if n == 4)
    flag = sum(c.ncls[:t4])
    for b in range(c.B):
        span = torch.tensor([c.fw * cell, c.fh * cell])
        boxes[b][:, :2] = torch.rand(c.M, 2, generator=g) * span * 1.2 + torch.tensor([pc0, pc1]) - 0.1 * span
        lab = torch.randint(-1, total + 1, (c.M,), generator=g)
        if len(c.ncls) == 1:                                  # one task: few foreign labels, so that it overflows max_objs
            lab = torch.where((lab < 0) | (lab >= total), torch.randint(0, total, (c.M,), generator=g), lab)
        cls = flag + (3 if b == 0 else 2)
        lab[188:197] = cls
        lab[c.M - 4:] = cls
        labels[b] = lab.to(c.label_dtype)
    return boxes, labels


def tgt_task_classes(name, b, t):
    """Per box of sample b its class within task t (-1: not the task's), as load_class has it."""
    c = TGT_CASES[name]
    lab = tgt_scene(name)[1][b].long() - sum(c.ncls[:t])
    return torch.where((lab >= 0) & (lab < c.ncls[t]), lab, torch.full_like(lab, -1))


# ---- det_loss: name -> (make_case key (B, H, W, K, ncls), vel)
LOSS_CASES = {
    "ncls431-K255": ((2, 5, 7, 255, (4, 3, 1)), True),
    "ncls431-K256-novel": ((2, 5, 7, 256, (4, 3, 1)), False),
    "T8-K257": ((2, 5, 7, 257, T8_NCLS), True),
    "K4096": ((1, 5, 7, 4096, (2, 4)), True),
    "K4096-novel": ((1, 3, 3, 4096, (1,)), False),
    "B65-3x3": ((65, 3, 3, 9, (4, 3, 1)), True),
}
LOSS_CROWD = (248, 264)        # live slots of slot 0's cell, either side of the 256-slot chunk (where K reaches that far)


@functools.lru_cache(maxsize=None)
def loss_case(name):
    key, vel = LOSS_CASES[name]
    c = TL.make_case(*key, vel=vel)
    K = key[3]
    lo, hi = LOSS_CROWD[0], min(LOSS_CROWD[1], K)
    if hi <= lo:
        return c
    inds, masks = c.inds.clone(), c.masks.clone()
    inds[..., lo:hi] = inds[..., :1]
    masks[..., lo:hi] = 1
    return dataclasses.replace(c, inds=inds, masks=masks)


# ---- det_post: name -> PostCase
@dataclasses.dataclass(frozen=True)
class PostCase:
    ncls: tuple
    H: int
    W: int
    max_num: int
    post: int
    kind: str = "circle"
    scene: str = "dense"
    B: int = 2
    pre: int = 1000
    dtype: torch.dtype = torch.float32
    min_radius: float = None          # one radius for every task instead of the reference's table
    peaks: tuple = None               # scene "peaks": candidates above the threshold per sample


NCLS4 = (3, 4, 1, 2)
POST_CASES = {f"K{k}-9x31": PostCase(NCLS4, 9, 31, k, min(k, 83)) for k in (1, 63, 64, 65, 128)}
POST_CASES.update({
    "N<64-2x3": PostCase(NCLS4, 2, 3, 500, 83, min_radius=0.5),
    "7x150-size-aware": PostCase(NCLS4, 7, 150, 500, 83, kind="size_aware_circle", B=1),
    "T1-bf16": PostCase((4,), 9, 31, 100, 83, dtype=torch.bfloat16),
    "T8-K-differs-4x40": PostCase(T8_NCLS, 4, 40, 500, 83, B=1),
    "survivors-63-64-65": PostCase((2, 3), 9, 31, 128, 83, scene="peaks", B=3, peaks=(63, 64, 65), min_radius=4.0),
    "post70-in-block2": PostCase(NCLS4, 9, 31, 128, 70, min_radius=0.01),
})
POST_CASES.update({f"rotate-pre{p}": PostCase(NCLS4, 9, 31, 128, 83, kind="rotate", B=1, pre=p) for p in (1, 63, 65)})


def post_setup(c):
    """(coder, test_cfg) of the reference head at cfg-A with the case's max_num / sizes, the per-task lists of the test
    configuration stretched over the case's tasks."""
    T = len(c.ncls)
    _, ref, tc = TP.head_setup(CFG_A, c.kind, post_max_size=c.post, pre_max_size=c.pre, nms_thr=0.2)
    coder = M.CenterPointBBoxCoder(pc_range=ref.pc_range, out_size_factor=ref.out_size_factor, voxel_size=ref.voxel_size,
                                   post_center_range=ref.post_center_range, max_num=c.max_num,
                                   score_threshold=ref.score_threshold)
    tc["min_radius"] = [c.min_radius] * T if c.min_radius is not None else (list(tc["min_radius"]) * 2)[:T]
    tc["thresh_scale"] = (list(tc["thresh_scale"]) * 2)[:T]
    return coder, tc


def peaks_heat(c, seed):
    """Per task a [B, ncls, H, W] heatmap on a -8 floor with exactly peaks[b] logits above the score threshold 0.1 in
    sample b: the strongest (6.0) in class 0 at one cell, the weakest (-0.5, score 0.38) in class 1 at the same cell --
    the same decoded centre, so the first candidate suppresses the last one, which for 65 candidates sits in the second
    64-row block -- and the others, pairwise distinct in (0, 5), at random (class, cell) places."""
    g = gen(seed)
    HW = c.H * c.W
    heats = []
    for n in c.ncls:
        heat = torch.full((c.B, n, c.H, c.W), -8.0)
        for b, cnt in enumerate(c.peaks):
            cell = int(torch.randint(0, HW, (1,), generator=g))
            free = torch.tensor([i for i in range(n * HW) if i not in (cell, HW + cell)])
            pos = free[torch.randperm(len(free), generator=g)[:cnt - 2]]
            flat = heat[b].view(-1)
            steps = torch.randperm(cnt - 2, generator=g).float() + torch.rand(cnt - 2, generator=g) * 0.5
            flat[pos] = steps * (5.0 / cnt) + 0.01
            flat[cell], flat[HW + cell] = 6.0, -0.5
        heats.append(heat)
    return heats


# ---- det_post: pairs of boxes of known IoU (x, y, dx, dy, yaw), the first one scoring higher
R2 = math.sqrt(2.0)
IOU_PAIRS = {
    "identical": ((1.0, 0.5, 3.0, 2.0, 0.0), (1.0, 0.5, 3.0, 2.0, 0.0), 1.0),
    "identical-yaw0.3": ((1.0, 0.5, 3.0, 2.0, 0.3), (1.0, 0.5, 3.0, 2.0, 0.3), 1.0),
    "shifted-half-side-x": ((0.0, 0.0, 4.0, 2.0, 0.0), (2.0, 0.0, 4.0, 2.0, 0.0), 1.0 / 3.0),
    "shifted-half-side-y": ((0.0, 0.0, 4.0, 2.0, 0.0), (0.0, 1.0, 4.0, 2.0, 0.0), 1.0 / 3.0),
    "touching-edge": ((0.0, 0.0, 2.0, 2.0, 0.0), (2.0, 0.0, 2.0, 2.0, 0.0), 0.0),
    "contained-flush": ((0.0, 0.0, 4.0, 4.0, 0.0), (1.0, 0.0, 2.0, 2.0, 0.0), 0.25),
    "quarter-turn": ((0.0, 0.0, 4.0, 2.0, 0.0), (0.0, 0.0, 4.0, 2.0, math.pi / 2), 1.0 / 3.0),
    "half-turn": ((0.5, 0.0, 4.0, 2.0, 0.0), (0.5, 0.0, 4.0, 2.0, math.pi), 1.0),
    "octagon-45": ((0.0, 0.0, 2.0, 2.0, 0.0), (0.0, 0.0, 2.0, 2.0, math.pi / 4), 1.0 / R2),
}


def pair_thresholds(iou):
    """(nms_thr per task, boxes kept per task): 1e-3 (relative) below the IoU the second box goes, 1e-3 above it stays;
    for IoU 0 the thresholds are 0 and 1e-3 and it stays under both (0 > 0 is false); at 1 and above every box stays."""
    if iou == 0.0:
        return [0.0, 1e-3, 1.0, 1.5], [2, 2, 2, 2]
    return [iou * (1 - 1e-3), iou * (1 + 1e-3), 1.0 if iou < 1.0 else 1.0 + 1e-3, 1.5], [1, 2, 2, 2]


# ---- rgb_loss: name -> (N, C, H, W)
RGB_CASES = {"2x4x186x202": (2, 4, 186, 202), "5x2x176x234": (5, 2, 176, 234), "1x1x177x700": (1, 1, 177, 700)}


# =====================================================================================================================
# GPU comparisons
# =====================================================================================================================
# ------------------------------------------------------------------------------------------------------------ seg_loss
@gpu
@pytest.mark.parametrize("name", list(SEG_ROWS_CASES))
def test_seg_loss_scan_turns(dev, name):
    """Loss, terms and gradient at element counts whose 256 T digit counters fill one scan turn exactly, spill 256
    counters into a second, and take three: test_seg_loss.compare, its bar unchanged."""
    P, Cn = SEG_ROWS_CASES[name]
    logits, labels, mask, _ = TS.case(P, Cn)
    hip, win = TS.device_case(P, Cn)
    TS.compare(f"seg_loss {name}: P = {P}, C = {Cn}, tiles {seg_tiles(P)}, scan turns {seg_scan_turns(P)}", logits, labels,
               mask, dev, hip, win)


@gpu
def test_seg_loss_sort_is_exact_in_the_second_turn(dev):
    """test_seg_loss.test_sort_is_exact's check on the two-turn case: the permutation is the stable descending sort of
    the device's own keys, which the carry between the scan's turns decides for every digit above the first turn."""
    P, Cn = SEG_ROWS_CASES[SEG_SORT_CASE]
    assert seg_scan_turns(P)[0] == 2
    TS.test_sort_is_exact(dev, P, Cn)
    n = TS.device_case(P, Cn)[1][0]
    print(f"\nseg_loss sort, P = {P}, C = {Cn}: {n} valid elements in stable descending order for every class")


@gpu
def test_seg_loss_channel_first_uint8_second_turn(dev):
    """C = 3, uint8 labels, [B, C, S] memory behind a permute view, B S = 131 073 with S odd."""
    c = SEG_PLANES
    B, S, Cn = c["B"], c["S"], c["Cn"]
    logits, labels, mask = seg_planes_inputs()
    assert labels.dtype == torch.uint8 and seg_scan_turns(B * S)[0] == 2 and S % 2 == 1
    mem = logits.reshape(B, S, Cn).permute(0, 2, 1).contiguous().to(dev)
    view = mem.permute(0, 2, 1).requires_grad_(True)
    assert not view.is_contiguous()
    y, m = labels.reshape(B, S).to(dev), mask.reshape(B, S).to(dev)
    loss = ops.seg_loss(view, y, m)
    loss.backward()
    hip = (loss.detach(), loss.terms, loss.n_valid, loss.n_present, view.grad.reshape(B * S, Cn))
    win = TS.window(view.detach(), y, m, dev)
    TS.compare(f"seg_loss channel-first uint8: B = {B}, S = {S}, C = {Cn}", logits, labels, mask, dev, hip, win)


@gpu
def test_seg_loss_cleared_tiles_and_a_class_without_foreground(dev):
    """Two scan turns with whole 2048-record tiles masked out (their records carry the invalid key only) either side of
    the turn boundary, and class 2 without a foreground element (G = 0: no Lovasz term, unit gradient 0)."""
    c = SEG_CLEARED
    logits, labels, mask = seg_cleared_inputs()
    valid = TS.valid_of(labels, mask, c["Cn"])
    assert seg_scan_turns(c["P"])[0] == 2 and int((labels[valid] == 2).sum()) == 0
    assert all(int(valid[t * SEG_TILE:(t + 1) * SEG_TILE].sum()) == 0 for t in c["tiles"])
    TS.compare(f"seg_loss cleared tiles {c['tiles']}: P = {c['P']}, C = {c['Cn']}", logits, labels, mask, dev)
    n, present, _, _ = TS.window(logits, labels, mask, dev)
    print(f"  n = {n}, classes present = {present}")
    assert present == 2 and n == int(valid.sum())


# --------------------------------------------------------------------------------------------------------- det_targets
@gpu
@pytest.mark.parametrize("name", list(TGT_CASES))
def test_det_targets_classes_2_and_3(dev, name):
    """Heatmaps, anno, inds and masks bit-exact against test_det_targets.oracle, tasks_ncls given explicitly."""
    c = TGT_CASES[name]
    tc = tgt_cfg(c)
    boxes, labels = tgt_scene(name)
    boxes, labels = [b.to(dev) for b in boxes], [l.to(dev) for l in labels]
    got = ops.det_targets(boxes, labels, c.ncls, tc, c.norm_bbox)
    ref = TT.oracle(boxes, labels, c.ncls, tc, c.norm_bbox)
    heat, anno, inds, masks = got.as_tuple()
    for t, n in enumerate(c.ncls):
        print(f"[det_targets:{name}] task {t} ({n} classes): live slots {int(ref[3][t].sum())} of {c.B} x {c.max_objs}, "
              f"heat pixels > 0 per class {[int((ref[0][t][:, k] > 0).sum()) for k in range(n)]}, "
              f"differing pixels {int((heat[t] != ref[0][t]).sum())}, anno bits equal {TT.same_bits(anno[t], ref[1][t])}, "
              f"inds equal {torch.equal(inds[t], ref[2][t])}, masks equal {torch.equal(masks[t], ref[3][t])}")
    assert got.anno.shape == (len(c.ncls), c.B, c.max_objs, c.cols + 1)
    assert [tuple(h.shape) for h in heat] == [(c.B, n, c.fh, c.fw) for n in c.ncls]
    TT.assert_matches_oracle(got, ref)
    # the cases are about classes 2 and 3: where at least five of a class's boxes get a slot, some are drawn
    for t, n in enumerate(c.ncls):
        for k in range(2, n):
            slots = [0] * c.B
            for b in range(c.B):
                cls = tgt_task_classes(name, b, t)
                first = int((cls >= 0).sum() - (cls >= k).sum())
                slots[b] = max(0, min(c.max_objs, first + int((cls == k).sum())) - first)
            peaks = [int((ref[0][t][b, k] == 1).sum()) for b in range(c.B)]
            print(f"[det_targets:{name}] task {t} class {k}: slots per sample {slots}, peaks {peaks}")
            assert all(p > 0 for p, s in zip(peaks, slots) if s >= 5), f"task {t}: no peak in class {k}"
            assert all(p == 0 for p, s in zip(peaks, slots) if s == 0), f"task {t}: class {k} drawn beyond max_objs"


# ------------------------------------------------------------------------------------------------------------ det_loss
@gpu
@pytest.mark.parametrize("name", list(LOSS_CASES))
def test_det_loss_paths(dev, name):
    """test_det_loss.compare (the comparison of its test_against_oracle), the bar unchanged."""
    key, vel = LOSS_CASES[name]
    c = loss_case(name)
    ora = TL.oracle(c.preds, c.heats, c.anno, c.inds, c.masks, c.cw, TL.WB)
    loss, terms, grads = TL.compare(f"det_loss {name}: B = {key[0]}, map {key[1]} x {key[2]}, K = {key[3]}, ncls = {key[4]}, "
                                    f"vel = {vel}", c, dev, ora)
    assert all(("vel" in g) == vel for g in grads) and c.anno.shape[-1] == (10 if vel else 8)
    if key[3] > LOSS_CROWD[0]:
        crowd = int(((c.inds == c.inds[..., :1]) & (c.masks != 0)).sum(-1).min())
        print(f"  live slots on slot 0's cell: at least {crowd} per (task, sample)")
        assert crowd >= min(LOSS_CROWD[1], key[3]) - LOSS_CROWD[0]


# ------------------------------------------------------------------------------------------------------------ det_post
def post_instance(c, dev, heats_of=None):
    """test_det_postprocess.instance with the case's coder; `heats_of(seed)` replaces the scene's heatmaps.  The margin
    rule is instance's: the next seed is drawn while a compared pair lies near its NMS threshold."""
    coder, tc = post_setup(c)
    if heats_of is None:
        preds, ref = TP.instance(c.B, c.H, c.W, c.scene, c.dtype, coder, tc, dev, ncls=list(c.ncls))
        return coder, tc, preds, ref
    for s in range(20):
        preds = TP.make_preds(c.B, c.H, c.W, "sparse", c.dtype, s, dev, ncls=list(c.ncls))
        for pd, h in zip(preds, heats_of(s)):
            pd[0]["heatmap"].copy_(h)
        ref, near = TP.oracle(preds, coder, tc, list(c.ncls), True)
        if not near:
            return coder, tc, preds, ref
    pytest.fail("no instance outside the NMS margin in 20 seeds")


def post_report(name, c, res, ref):
    counts = res.counts.cpu().tolist()
    per_task = [[int(((res.labels[b, :counts[b]] >= sum(c.ncls[:t])) & (res.labels[b, :counts[b]] < sum(c.ncls[:t + 1]))).sum())
                 for t in range(len(c.ncls))] for b in range(c.B)]
    print(f"[det_post:{name}] kept per sample {counts} (oracle {[len(r[2]) for r in ref]}), per task {per_task}, "
          f"plan {post_plan(c.H, c.W, c.ncls, c.max_num)}")
    return per_task


@gpu
@pytest.mark.parametrize("name", list(POST_CASES))
def test_det_post_paths(dev, name):
    """test_det_postprocess.assert_matches against its oracle, under instance's margin rule."""
    c = POST_CASES[name]
    heats_of = (lambda s: peaks_heat(c, s)) if c.scene == "peaks" else None
    coder, tc, preds, ref = post_instance(c, dev, heats_of)
    res = ops.det_postprocess(preds, coder, tc, list(c.ncls), True)
    per_task = post_report(name, c, res, ref)
    TP.assert_matches(res, ref, c.dtype, c.post, len(c.ncls))
    labels = torch.cat([r[2] for r in ref])
    if any(n >= 3 for n in c.ncls) and c.max_num > 1 and c.scene == "dense" and c.pre > 1:
        # classes 2 and 3 of a task come back: cls = idx / HW above 1
        for t, n in enumerate(c.ncls):
            if n >= 3:
                assert int(((labels >= sum(c.ncls[:t]) + 2) & (labels < sum(c.ncls[:t + 1]))).sum()) > 0, \
                    f"task {t}: no detection of class 2 or 3"
    if c.scene == "peaks":
        cand = [[len(d[2]) for d in TP.oracle_decode(pd[0], coder, True)] for pd in preds]
        print(f"  candidates after the filters per task and sample: {cand}")
        assert all(row == list(c.peaks) for row in cand)
        assert all(per_task[b][t] < c.peaks[b] for b in range(c.B) for t in range(len(c.ncls))), "nothing was suppressed"
    if name == "post70-in-block2":
        assert c.post > 64 and all(k == c.post for row in per_task for k in row), "post_max_size was not reached"
    if c.kind == "rotate":
        assert all(k <= c.pre for row in per_task for k in row)
        if c.pre > 1:
            assert any(1 < k < c.pre for row in per_task for k in row), "rotated NMS suppressed nothing or everything"


def pair_preds(a, b, T, dev):
    """Head outputs on a 2 x 3 map (one class) that decode, with the identity coder and dims taken as they are, to box
    `a` from cell (0, 0) with score sigmoid(3) and box `b` from cell (0, 1) with sigmoid(2); every other cell stays
    under the score threshold.  The T tasks share the tensors."""
    H, W = 2, 3
    heat = torch.full((1, 1, H, W), -8.0)
    z = lambda n: torch.zeros(1, n, H, W)           # noqa: E731
    reg, height, dim, rot = z(2), z(1), torch.ones(1, 3, H, W), z(2)
    rot[:, 1] = 1.0
    for k, (x, y, dx, dy, yaw) in enumerate((a, b)):
        heat[0, 0, 0, k] = 3.0 - k
        reg[0, :, 0, k] = torch.tensor([x - k, y])
        dim[0, :, 0, k] = torch.tensor([dx, dy, 1.0])
        rot[0, :, 0, k] = torch.tensor([math.sin(yaw), math.cos(yaw)], dtype=torch.float64).float()
    p = {k: v.to(dev) for k, v in dict(heatmap=heat, reg=reg, height=height, dim=dim, rot=rot).items()}
    return [[p] for _ in range(T)]


PAIR_CODER = dict(pc_range=[0.0, 0.0], out_size_factor=1, voxel_size=[1.0, 1.0], post_center_range=None, max_num=6,
                  score_threshold=0.5)


@gpu
@pytest.mark.parametrize("name", list(IOU_PAIRS))
def test_det_post_rotated_iou_closed_forms(dev, name):
    """Two boxes of known IoU under rotated NMS, one task per threshold: the thresholds sit 1e-3 (relative) from the
    closed form, five times the 2e-4 the oracle's margin rule keeps clear, so the keep lists are those of the closed
    form -- and of the float64 oracle, which assert_matches compares as well."""
    a, b, iou = IOU_PAIRS[name]
    thrs, want = pair_thresholds(iou)
    T = len(thrs)
    coder = M.CenterPointBBoxCoder(**PAIR_CODER)
    tc = dict(nms_type="rotate", nms_thr=thrs, pre_max_size=6, post_max_size=6)
    preds = pair_preds(a, b, T, dev)
    ref, _ = TP.oracle(preds, coder, tc, [1] * T, False)
    res = ops.det_postprocess(preds, coder, tc, [1] * T, False)
    n = int(res.counts[0])
    got = [int((res.labels[0, :n] == t).sum()) for t in range(T)]
    dec = TP.oracle_decode(preds[0][0], coder, False)[0][0]
    o_iou = TP.rotated_iou(dec[0, [0, 1, 3, 4, 6]].double().numpy(), dec[1, [0, 1, 3, 4, 6]].double().numpy())
    print(f"[det_post:pair {name}] closed-form IoU {iou:.9f}, float64 clip of the decoded boxes {o_iou:.9f}, nms_thr {thrs}, "
          f"kept per task {got}, expected {want}, oracle {[int((ref[0][2] == t).sum()) for t in range(T)]}")
    assert tuple(dec.shape) == (2, 7) and abs(o_iou - iou) <= 1e-6
    assert got == want
    TP.assert_matches(res, ref, torch.float32, 6, T)


# ------------------------------------------------------------------------------------------------------------ rgb_loss
@gpu
@pytest.mark.parametrize("name", list(RGB_CASES))
def test_rgb_loss_shapes(dev, name):
    """test_rgb_loss.compare, its bar unchanged."""
    shape = RGB_CASES[name]
    pred, target = TR.make_inputs(shape, seed=11)
    ora = TR.oracle(pred, target)
    assert float(ora[2].min()) > 0.1, "a per-scale value near the relu: the inputs are not what the bar was stated for"
    scales = [(s.H, s.W, s.ty, s.tx, s.lrows, s.lcols) for s in rgb_scales(*shape[2:])]
    TR.compare(f"rgb_loss [N, C, H, W] = {shape}, scales (H, W, ty, tx, last rows, last columns) {scales}", pred, target,
               ora, dev)


# =====================================================================================================================
# CPU tests: what the cases reach, the mirrors against the library, the crafted pairs
# =====================================================================================================================
def _unreached(required, reached):
    return sorted(str(r) for r in set(required) - set(reached))


def test_seg_loss_cases_reach_every_regime():
    reached = set()
    for name, (P, Cn) in SEG_ROWS_CASES.items():
        turns, last = seg_scan_turns(P)
        assert seg_valid(1, P, Cn) and Cn == 2
        reached.add(f"turns{turns}")
        reached |= {k for k, v in (("one-turn-full", turns == 1 and last == SEG_SCAN_TURN),
                                   ("second-turn-256", turns == 2 and last == 256),
                                   ("sort-check-two-turns", name == SEG_SORT_CASE and turns == 2)) if v}
        # make_case at C = 2 labels every element 0: class 1 has no foreground (G = 0) in each of these
        logits, labels, mask, valid = TS.case(P, Cn)
        if int((labels[valid] == 1).sum()) == 0:
            reached.add(f"G0-turns{turns}")
    c = SEG_PLANES
    logits, labels, mask = seg_planes_inputs()
    if labels.dtype == torch.uint8 and c["S"] % 2 and c["Cn"] == 3 and seg_scan_turns(c["B"] * c["S"])[0] == 2:
        reached.add("planes-u8-C3-S-odd-two-turns")
    assert 131072 < c["B"] * c["S"] <= 131072 + 2048
    assert seg_valid(c["B"], c["S"], c["Cn"], _capi.VAMP_SEG_PLANES, _capi.VAMP_U8)
    c = SEG_CLEARED
    logits, labels, mask = seg_cleared_inputs()
    valid = TS.valid_of(labels, mask, c["Cn"])
    tiles, turns = seg_tiles(c["P"]), seg_scan_turns(c["P"])[0]
    empty = [t for t in range(tiles) if int(valid[t * SEG_TILE:(t + 1) * SEG_TILE].sum()) == 0]
    assert empty == sorted(c["tiles"])
    per_turn = SEG_SCAN_TURN // SEG_RADIX                       # tiles whose counters of ONE digit fill a turn
    if turns == 2 and any(t < per_turn for t in empty) and any(t >= per_turn for t in empty):
        reached.add("cleared-tiles-two-turns")
    if turns == 2 and int((labels[valid] == 2).sum()) == 0 and all(int((labels[valid] == k).sum()) > 0 for k in (0, 1)):
        reached.add("G0-beside-present-classes-two-turns")
    required = {"turns1", "turns2", "turns3", "one-turn-full", "second-turn-256", "sort-check-two-turns", "G0-turns2",
                "planes-u8-C3-S-odd-two-turns", "cleared-tiles-two-turns", "G0-beside-present-classes-two-turns"}
    assert not _unreached(required, reached), f"seg_loss regimes no case reaches: {_unreached(required, reached)}"
    # the issue's arithmetic, and the largest shape of test_seg_loss
    assert (seg_tiles(131072), seg_tiles(131073), seg_tiles(262145)) == (64, 65, 129)
    assert seg_scan_turns(70001) == (1, 35 * 256) and seg_scan_turns(640000)[0] == 5


def _runs_across(cls, c, k):
    """Whether boxes [k - 1, k] are both of class c: a run of the class across box index k."""
    return 0 < k < len(cls) and int(cls[k - 1]) == c and int(cls[k]) == c


def test_det_targets_cases_reach_every_regime():
    reached = set()
    for name, c in TGT_CASES.items():
        assert tgt_valid(c.B, c.M, c.ncls, c.cols, c.cols + 1, c.max_objs, c.fh, c.fw), name
        ntx, nty, lw, lh = tgt_grid(c.fh, c.fw)
        reached |= {f"M{c.M}", f"cols{c.cols}", "i64" if c.label_dtype == torch.int64 else "i32", f"table{c.ncls}",
                    f"map{c.fh}x{c.fw}", f"norm_bbox{int(c.norm_bbox)}"}
        reached |= {f"ncls{n}" for n in c.ncls}
        reached |= {k for k, v in (("fw<32", c.fw < TGT_TILE_W), ("fw-two-tiles-partial", ntx == 2 and lw < TGT_TILE_W),
                                   ("fh<8", c.fh < TGT_TILE_H), ("fh-tiles-partial", nty > 1 and lh < TGT_TILE_H),
                                   ("fh-tiles-whole", nty > 1 and lh == TGT_TILE_H),
                                   ("T8-every-ncls", len(c.ncls) == 8 and set(c.ncls) == {1, 2, 3, 4}),
                                   ("label-chunks2", cdiv(c.M, TGT_BLOCK) == 2)) if v}
        for b, t in itertools.product(range(c.B), range(len(c.ncls))):
            cls = tgt_task_classes(name, b, t)
            counts = [int((cls == k).sum()) for k in range(4)]
            ntask = sum(counts)
            for k in (2, 3):
                if c.ncls[t] <= k:
                    assert counts[k] == 0
                    continue
                assert counts[k] > 0, (name, b, t, k)
                reached |= {f"class{k}-across-{w}" for w, at in (("wave", 192), ("chunk", 256)) if _runs_across(cls, k, at)}
                first = sum(counts[:k])
                if first < c.max_objs < first + counts[k]:
                    reached.add(f"truncated-inside-class{k}")
            if ntask > TGT_BLOCK:
                reached.add("record-chunks2")
            if ntask < c.max_objs:
                reached.add("slots-left-over")
    required = ({f"M{m}" for m in (255, 256, 257)} | {"cols7", "cols9", "i32", "i64", "table(3, 4, 1)", "table(4,)", "map5x33",
                                                       "map9x31", "map40x7", "ncls1", "ncls2", "ncls3", "ncls4", "fw<32",
                                                       "fw-two-tiles-partial", "fh<8", "fh-tiles-partial", "fh-tiles-whole",
                                                       "T8-every-ncls", "label-chunks2", "class2-across-wave",
                                                       "class3-across-wave", "class2-across-chunk", "class3-across-chunk",
                                                       "truncated-inside-class2", "truncated-inside-class3", "slots-left-over",
                                                       "norm_bbox0", "norm_bbox1"})
    assert not _unreached(required, reached), f"det_targets regimes no case reaches: {_unreached(required, reached)}"
    assert tgt_grid(5, 33) == (2, 1, 1, 5) and tgt_grid(9, 31) == (1, 2, 31, 1) and tgt_grid(40, 7) == (1, 5, 7, 8)


def test_det_loss_cases_reach_every_regime():
    reached = set()
    for name, (key, vel) in LOSS_CASES.items():
        B, H, W, K, ncls = key
        code = 10 if vel else 8
        assert loss_valid(B, H, W, K, ncls, code, int(vel)), name
        p = loss_plan(B, H, W, K, ncls, code)
        reached |= {f"K{K}", f"vel{int(vel)}", f"table{ncls}", f"slot-turns{p.slot_turns}"} | {f"ncls{n}" for n in ncls}
        reached |= {k for k, v in (("T8", len(ncls) == 8), ("B65-3x3", (B, H, W) == (65, 3, 3)),
                                   ("box-turns2", p.box_turns == 2),
                                   ("heat-chunks>1", max(p.heat_chunks) > 1), ("K-at-the-LDS-cap", K == LOSS_MAX_OBJS)) if v}
        c = loss_case(name)
        same = (c.inds == c.inds[..., :1]) & (c.masks != 0)
        if K > 256 and bool(same[..., LOSS_CROWD[0]:256].all()) and bool(same[..., 256:min(K, LOSS_CROWD[1])].all()):
            reached.add("crowd-both-sides-of-chunk")
        if K == 256 and bool(same[..., LOSS_CROWD[0]:256].all()):
            reached.add("crowd-fills-chunk-end")
    required = {"K255", "K256", "K257", "K4096", "vel0", "vel1", "table(4, 3, 1)", "ncls1", "ncls2", "ncls3", "ncls4", "T8",
                "B65-3x3", "box-turns2", "slot-turns1", "slot-turns2", "slot-turns16", "K-at-the-LDS-cap",
                "crowd-both-sides-of-chunk", "crowd-fills-chunk-end"}
    assert not _unreached(required, reached), f"det_loss regimes no case reaches: {_unreached(required, reached)}"
    assert loss_plan(65, 3, 3, 9, (4, 3, 1), 10).box_turns == 2 and loss_plan(64, 3, 3, 9, (1,), 10).box_turns == 1
    assert loss_plan(2, 128, 128, 500, TL.NCLS6, 10).heat_turns == (1, 1, 1, 1, 1, 1)        # what the suite ran before


def test_det_post_cases_reach_every_regime():
    reached = set()
    for name, c in POST_CASES.items():
        rotate = c.kind == "rotate"
        assert post_valid(c.B, c.H, c.W, c.ncls, c.max_num, c.post, c.pre, rotate), name
        p = post_plan(c.H, c.W, c.ncls, c.max_num)
        reached |= {f"kind-{c.kind}", f"T{len(c.ncls)}", f"table{c.ncls}"}
        if all(k < n for k, n in zip(p.K, p.N)):
            reached |= {f"K{k}<N" for k in p.K}
        reached |= {k for k, v in (("N<64", max(p.N) < 64), ("K=N-differs-per-task", len(set(p.K)) > 1 and max(p.N) < 64),
                                   ("7x150", (c.H, c.W) == (7, 150)), ("H!=W-above-4x5", c.H != c.W and c.H * c.W > 20),
                                   ("K-differs-blocks-unvisited", any(cdiv(k, 64) < p.nblk for k in p.K) and p.nblk > 1),
                                   ("cls3-decoded", max(c.ncls) == 4), ("cls2-decoded", 3 in c.ncls),
                                   ("KS>K", any(ks > k for ks, k in zip(p.KS, p.K))),
                                   ("KS=K", any(ks == k for ks, k in zip(p.KS, p.K))),
                                   ("gather-chunk>1", max(p.chunk) > 1), ("nblk8", p.nblk == 8), ("nblk2", p.nblk == 2),
                                   ("post>64", c.post > 64 and min(p.K) > c.post), ("bf16", c.dtype == torch.bfloat16)) if v}
        if rotate:
            reached.add(f"rotate-pre{c.pre}")
            assert min(c.pre, max(p.K)) <= 130, "the float64 rotated oracle is quadratic Python"
        if c.scene == "peaks":
            reached |= {f"survivors{n}" for n in c.peaks}
            assert p.nblk == 2 and all(n <= min(p.K) for n in c.peaks) and c.kind == "circle" and all(n >= 2 for n in c.ncls)
            for s in (0, 1):                            # exactly peaks[b] logits above the threshold, the extremes on one cell
                for heat in peaks_heat(c, s):
                    assert [int((heat[b] > math.log(1 / 9)).sum()) for b in range(c.B)] == list(c.peaks)
                    top = heat.flatten(2).argmax(2)
                    assert bool((heat.flatten(2).gather(2, top[..., None])[:, 0, 0] == 6.0).all())
                    assert bool((heat[:, 1].flatten(1).gather(1, top[:, :1])[:, 0] == -0.5).all())
    required = ({f"K{k}<N" for k in (1, 63, 64, 65, 128)} | {f"survivors{n}" for n in (63, 64, 65)}
                | {f"rotate-pre{p}" for p in (1, 63, 65)}
                | {"kind-circle", "kind-size_aware_circle", "kind-rotate", "T1", "T8", "table(3, 4, 1, 2)", "N<64",
                   "K=N-differs-per-task", "7x150", "H!=W-above-4x5", "K-differs-blocks-unvisited", "cls2-decoded",
                   "cls3-decoded", "KS>K", "KS=K", "gather-chunk>1", "nblk8", "nblk2", "post>64", "bf16"})
    assert not _unreached(required, reached), f"det_post regimes no case reaches: {_unreached(required, reached)}"
    p = post_plan(4, 40, T8_NCLS, 500)
    assert p.K == (160, 320, 480, 500, 500, 480, 320, 160) and (p.KP, p.nblk) == (512, 8)
    assert post_plan(2, 3, NCLS4, 500).K == (18, 24, 6, 12) and post_plan(9, 31, NCLS4, 1).KS == (1, 1, 1, 1)


def test_rgb_loss_cases_reach_every_regime():
    reached = set()
    for name, (N, Cn, H, W) in RGB_CASES.items():
        assert rgb_valid(N, Cn, H, W), name
        sc = rgb_scales(H, W)
        reached |= {f"C{Cn}", f"N{N}"}
        reached |= {k for k, v in (("N>4", N > 4), ("pairs>waves", N * RGB_SCALES > 4),
                                   ("valid-width-whole-tiles", (W - RGB_REACH) % RGB_TW == 0),
                                   ("valid-height-whole-tiles", (H - RGB_REACH) % RGB_TH == 0),
                                   ("last-tile-owns-42-columns", sc[0].lcols == RGB_TW + RGB_REACH),
                                   ("last-tile-owns-26-rows", sc[0].lrows == RGB_TH + RGB_REACH),
                                   ("last-tile-owns-11-columns", any(s.lcols == RGB_REACH + 1 for s in sc)),
                                   ("last-tile-owns-11-rows", any(s.lrows == RGB_REACH + 1 for s in sc)),
                                   ("non-square-3x", W >= 3 * H or H >= 3 * W),
                                   ("odd-side-pooled", any(s.H % 2 or s.W % 2 for s in sc[:4])),
                                   ("last-scale-one-window", sc[4].H == 11 or sc[4].W == 11),
                                   ("partials>64", Cn * sc[0].tx * sc[0].ty > 64)) if v}
        assert all(RGB_REACH < s.lcols <= RGB_TW + RGB_REACH and RGB_REACH < s.lrows <= RGB_TH + RGB_REACH for s in sc)
    required = {"C1", "C2", "C4", "N5", "N>4", "pairs>waves", "valid-width-whole-tiles", "valid-height-whole-tiles",
                "last-tile-owns-42-columns", "last-tile-owns-26-rows", "last-tile-owns-11-columns", "last-tile-owns-11-rows",
                "non-square-3x", "odd-side-pooled", "last-scale-one-window", "partials>64"}
    assert not _unreached(required, reached), f"rgb_loss regimes no case reaches: {_unreached(required, reached)}"
    s0 = rgb_scales(186, 202)[0]
    assert (s0.ty, s0.tx, s0.lrows, s0.lcols) == (11, 6, 26, 42)
    s0 = rgb_scales(177, 700)[0]
    assert (s0.ty, s0.tx, s0.lrows, s0.lcols) == (11, 22, 17, 28)


# ----------------------------------------------------------------------------------- the mirrors against the library
@pytest.fixture(scope="module")
def lib():
    from vampire_amd.build import build_library
    build_library(verbose=False)
    return _capi.load()


def test_seg_loss_host_answers_match_the_mirror(lib):
    sizes = [(1, 1), (1, 2047), (1, 2048), (1, 2049), (1, 70001), (1, 131072), (1, 131073), (3, 43691), (1, 262145),
             (6, 640000), (2, 25600000), (1, (1 << 31) - 1), (1, 1 << 31), (1 << 16, 1 << 15), (1 << 16, (1 << 15) - 1),
             (0, 5), (5, 0)]
    n = 0
    for (B, S), Cn, layout, label in itertools.product(sizes, (1, 2, 3, 18, 32, 33),
                                                       (_capi.VAMP_SEG_ROWS, _capi.VAMP_SEG_PLANES, 2),
                                                       SEG_LABELS + (_capi.VAMP_F32,)):
        d = _capi.VampSegLossDesc(B, S, Cn, layout, label, 0, 1.0, 1.0)
        kw = dict(layout=layout, label=label)
        assert lib.vamp_seg_loss_workspace_bytes(C.byref(d)) == seg_workspace(B, S, Cn, **kw), (B, S, Cn, layout, label)
        assert lib.vamp_seg_loss_kept_bytes(C.byref(d)) == seg_kept(B, S, Cn, **kw), (B, S, Cn, layout, label)
        n += seg_valid(B, S, Cn, **kw)
    assert n > 100 and seg_workspace(2, 25600000, 18) > 1 << 33        # 14.7 GB: no test could allocate it


def _post_desc(B, H, W, ncls, max_num, post, pre, rotate):
    d = _capi.VampDetDesc()
    d.B, d.T, d.H, d.W = B, len(ncls), H, W
    for t, n in enumerate(ncls):
        d.ncls[t] = n
    d.max_num, d.pre_max_size, d.post_max_size = max_num, pre, post
    d.nms_kind = _capi.VAMP_NMS_ROTATE if rotate else _capi.VAMP_NMS_CIRCLE
    d.in_dtype, d.has_vel, d.norm_bbox = _capi.VAMP_F32, 1, 1
    return d


def test_det_post_host_answers_match_the_mirror(lib):
    maps = [(1, 1), (2, 3), (4, 5), (9, 31), (7, 150), (4, 40), (128, 128), (200, 200), (4096, 4096), (23170, 23170),
            (16384, 32768)]
    tables = [(1,), (4,), NCLS4, (1, 2, 2, 1, 2, 2), T8_NCLS, (5,), (0, 1), ()]
    n = 0
    for (H, W), ncls, max_num, post, B in itertools.product(maps, tables, (1, 63, 64, 65, 128, 500, 1024, 1025),
                                                            (1, 70, 83, 2000), (1, 3, 1 << 20)):
        if not 1 <= len(ncls) <= 8:
            continue
        for rotate, pre in ((False, 0), (True, 0), (True, 65)):
            d = _post_desc(B, H, W, ncls, max_num, post, pre, rotate)
            want = post_workspace(B, H, W, ncls, max_num, post, pre, rotate)
            assert lib.vamp_det_workspace_bytes(C.byref(d)) == want, (B, H, W, ncls, max_num, post, pre, rotate)
            n += want > 0
    assert n > 1000 and post_workspace(1 << 20, 128, 128, (1, 2, 2, 1, 2, 2), 500, 83) > 1 << 38
    for name, c in POST_CASES.items():
        d = _post_desc(c.B, c.H, c.W, c.ncls, c.max_num, c.post, c.pre, c.kind == "rotate")
        assert lib.vamp_det_workspace_bytes(C.byref(d)) == post_workspace(c.B, c.H, c.W, c.ncls, c.max_num, c.post) > 0, name


def _loss_desc(B, H, W, K, ncls, code, has_vel):
    d = _capi.VampDetLossDesc()
    d.B, d.T, d.H, d.W = B, len(ncls), H, W
    for t, n in enumerate(ncls):
        d.ncls[t] = n
    d.code, d.max_objs, d.has_vel, d.loss_bbox_weight = code, K, has_vel, TL.WB
    for k in range(code if code in (8, 10) else 0):
        d.code_weights[k] = 1.0
    return d


def test_det_loss_host_answers_match_the_mirror(lib):
    maps = [(1, 1), (3, 3), (5, 7), (33, 65), (128, 128), (200, 200), (1024, 1024), (8192, 8192), (8193, 4), (0, 4)]
    tables = [(1,), (4, 3, 1), (2, 4), TL.NCLS6, T8_NCLS, (5, 1), (0,)]
    n = 0
    for (H, W), ncls, K, B, (code, vel) in itertools.product(maps, tables, (1, 255, 256, 257, 500, 4096, 4097, 0),
                                                             (1, 2, 64, 65, 4096, 4097), ((10, 1), (8, 0), (10, 0), (9, 1))):
        d = _loss_desc(B, H, W, K, ncls, code, vel)
        want = loss_workspace(B, H, W, K, ncls, code, vel)
        assert lib.vamp_det_loss_workspace_bytes(C.byref(d)) == want, (B, H, W, K, ncls, code, vel)
        n += want > 0
    assert n > 500 and loss_valid(64, 1024, 1024, 500, TL.NCLS6, 10, 1)
    assert not loss_valid(4096, 1024, 1024, 500, TL.NCLS6, 10, 1)        # more than 2^22 chunks
    for name, (key, vel) in LOSS_CASES.items():
        B, H, W, K, ncls = key
        assert lib.vamp_det_loss_workspace_bytes(C.byref(_loss_desc(B, H, W, K, ncls, 10 if vel else 8, int(vel)))) > 0, name


def _tgt_desc(B, M_, ncls, cols, code, max_objs, fh, fw, label):
    d = TT._desc(B=B, T=len(ncls), M=M_, box_cols=cols, code=code, max_objs=max_objs, fh=fh, fw=fw, label_dtype=label)
    for t in range(8):
        d.ncls[t] = ncls[t] if t < len(ncls) else 0
    return d


def test_det_targets_host_answers_match_the_mirror(lib):
    tables = [(1,), (4,), (3, 4, 1), TL.NCLS6, T8_NCLS, (5,), (1, 0)]
    n = 0
    for ncls, (fh, fw), M_, max_objs, B, (cols, code), label in itertools.product(
            tables, ((1, 1), (5, 33), (40, 7), (128, 128), (8192, 8192), (8193, 1), (4, 0)),
            (0, 255, 257, 1 << 20, (1 << 20) + 1),
            (1, 30, 500, 8192, 8193), (1, 2, 4096, 4097), ((9, 10), (7, 8), (7, 10), (8, 9)),
            (_capi.VAMP_I64, _capi.VAMP_I32, _capi.VAMP_U8)):
        d = _tgt_desc(B, M_, ncls, cols, code, max_objs, fh, fw, label)
        want = tgt_workspace(B, M_, ncls, cols, code, max_objs, fh, fw, label=label)
        assert lib.vamp_det_targets_workspace_bytes(C.byref(d)) == want, (B, M_, ncls, cols, code, max_objs, fh, fw, label)
        n += want > 0
    assert n > 1000
    for name, c in TGT_CASES.items():
        code = _capi.VAMP_I64 if c.label_dtype == torch.int64 else _capi.VAMP_I32
        d = _tgt_desc(c.B, c.M, c.ncls, c.cols, c.cols + 1, c.max_objs, c.fh, c.fw, code)
        assert lib.vamp_det_targets_workspace_bytes(C.byref(d)) > 0, name


def test_rgb_loss_host_answers_match_the_mirror(lib):
    sides = (175, 176, 177, 186, 192, 202, 234, 700, 1600, 16384, 16385)
    n = 0
    for H, W, N, Cn in itertools.product(sides, sides, (0, 1, 2, 5, 6, 64), (0, 1, 2, 3, 4, 5)):
        d = _capi.VampRgbLossDesc(N, Cn, H, W, 1.0, 0.01, 0.03)
        assert lib.vamp_rgb_loss_workspace_bytes(C.byref(d)) == rgb_workspace(N, Cn, H, W), (N, Cn, H, W)
        n += rgb_valid(N, Cn, H, W)
    assert n > 500 and rgb_workspace(1, 4, 16384, 16384) > 1 << 33 and not rgb_valid(2, 4, 16384, 16384)


# ---------------------------------------------------------------------------------------------------- the crafted pairs
def test_crafted_pairs_have_their_closed_form_iou():
    """The float64 clip of test_det_postprocess on every crafted pair against its closed form; the thresholds around it
    stand clear of the oracle's 2e-4 margin; and the pairs are the degenerate ones: equal yaw or a quarter / half turn
    (parallel edges, shared boundaries) and the octagon."""
    seen = set()
    for name, (a, b, iou) in IOU_PAIRS.items():
        got = TP.rotated_iou(a, b)
        assert abs(got - iou) <= 1e-12, (name, got, iou)
        assert abs(TP.rotated_iou(b, a) - iou) <= 1e-12, name
        thrs, want = pair_thresholds(iou)
        keep, near = zip(*[TP.rotate_nms([a, b], thr, 6, 6, margin=2e-4) for thr in thrs])
        assert [len(k) for k in keep] == want, (name, keep)
        assert not any(near[1:]) and (iou == 0.0 or not near[0]), (name, near)
        assert all(abs(thr - iou) >= 4.99 * 2e-4 * thr for thr in thrs[:2] if iou > 0), name
        turn = (b[4] - a[4]) / (math.pi / 2)
        seen.add("identical" if a == b else {0.0: "equal-yaw", 1.0: "quarter-turn", 2.0: "half-turn", 0.5: "45-degrees"}[turn])
        # shared boundary: an edge of one box lies on an edge line of the other
        ca, cb = TP.rect_corners(*a), TP.rect_corners(*b)
        on = 0
        for p, q in zip(ca, ca[1:] + ca[:1]):
            for r, s in zip(cb, cb[1:] + cb[:1]):
                side = lambda v: (s[0] - r[0]) * (v[1] - r[1]) - (s[1] - r[1]) * (v[0] - r[0])       # noqa: E731
                on += abs(side(p)) < 1e-9 and abs(side(q)) < 1e-9
        if on:
            seen.add("shared-boundary")
        if iou == 0.0:
            assert on >= 1 and math.hypot(a[0] - b[0], a[1] - b[1]) == a[2] / 2 + b[2] / 2
    assert seen == {"identical", "equal-yaw", "quarter-turn", "half-turn", "45-degrees", "shared-boundary"}
    assert IOU_PAIRS["octagon-45"][2] == pytest.approx(2 * (R2 - 1) / (4 - 2 * R2), abs=1e-12)
