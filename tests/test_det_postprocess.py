"""Detection post-processing on the device (ops.det_postprocess / BEVDepthHead.get_bboxes_device over the HIP
kernels of det_post.hip) against a host oracle: the reference head's get_bboxes (bev_depth_head.py:381-494)
with a deterministic top-K (score descending, then flat index ascending -- torch.topk leaves the order of ties
undefined), decode()'s own arithmetic, multitask.circle_nms / size_aware_circle_nms and a float64 restatement
of rotated-rectangle IoU (Sutherland-Hodgman clip + shoelace) with greedy NMS.

Margin rule: an NMS decision near its threshold could flip on an ulp of a transcendental (cos / sin / exp /
atan2 on another device, fp32 against float64 IoU).  The generators reject every instance in which a pair the
greedy walk compares lies within 1e-4 (relative) of the threshold -- 2e-4 for rotated IoU, computed in fp32 on the device -- and draw the next
seed instead, so the keep lists are exact."""
import ctypes as C
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, ops                           # noqa: E402
from vampire_amd import multitask as M                       # noqa: E402
from vampire_amd.build import build_library                  # noqa: E402
from vampire_amd.config import CFG_A, CFG_B, CFG_TINY        # noqa: E402

NCLS = [t["num_class"] for t in M.TASKS]
EPS = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


# ----------------------------------------------------------------------------- rotated IoU, float64
def rect_corners(x, y, dx, dy, yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return [(x + ox * c - oy * s, y + ox * s + oy * c)
            for ox, oy in ((-dx / 2, -dy / 2), (dx / 2, -dy / 2), (dx / 2, dy / 2), (-dx / 2, dy / 2))]


def _clip(poly, a, b):
    """Sutherland-Hodgman: the part of `poly` on the left of the directed line a -> b."""
    side = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
    out = []
    for k in range(len(poly)):
        p, q = poly[k], poly[(k + 1) % len(poly)]
        sp, sq = side(p), side(q)
        if sp >= 0:
            out.append(p)
        if (sp >= 0) != (sq >= 0):
            t = sp / (sp - sq)
            out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    return out


def _area(poly):
    return 0.5 * abs(sum(poly[k][0] * poly[(k + 1) % len(poly)][1] - poly[(k + 1) % len(poly)][0] * poly[k][1]
                         for k in range(len(poly))))


def rotated_iou(b1, b2):
    """IoU of two BEV boxes (x, y, dx, dy, yaw): intersection / max(union, 1e-8); a box with a side <= 0
    overlaps nothing."""
    b1, b2 = [float(v) for v in b1], [float(v) for v in b2]
    if min(b1[2], b1[3], b2[2], b2[3]) <= 0:
        return 0.0
    poly = rect_corners(*b1)
    clipper = rect_corners(*b2)
    for k in range(4):
        if not poly:
            break
        poly = _clip(poly, clipper[k], clipper[(k + 1) % 4])
    inter = _area(poly) if len(poly) >= 3 else 0.0
    return inter / max(b1[2] * b1[3] + b2[2] * b2[3] - inter, 1e-8)


def rotate_nms(bev, thr, pre_max, post_max, margin=None):
    """Greedy NMS by rotated IoU > thr over the first pre_max rows of bev [n, 5] (float64); returns the kept
    rows and whether a compared pair lay within `margin` (relative) of thr."""
    bev = np.asarray(bev, dtype=np.float64)[:pre_max]
    n = len(bev)
    rad = 0.5 * np.hypot(bev[:, 2], bev[:, 3])
    alive, keep, near = np.ones(n, bool), [], False
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) == post_max:
            break
        js = np.nonzero(alive[i + 1:])[0] + i + 1
        reach = np.hypot(bev[js, 0] - bev[i, 0], bev[js, 1] - bev[i, 1]) <= rad[js] + rad[i] + 1e-6
        for j in js[reach]:
            iou = rotated_iou(bev[i], bev[j])
            if margin is not None and abs(iou - thr) <= margin * max(thr, 1e-6):
                near = True
            if iou > thr:
                alive[j] = False
    return keep, near


# ----------------------------------------------------------------------------- the host oracle
def det_order(flat, K):
    """Flat indices of the top K scores: score descending, then index ascending; a NaN ranks first."""
    v = flat.double().numpy()
    key = np.where(np.isnan(v), np.inf, v)
    return torch.from_numpy(np.lexsort((np.arange(len(v)), -key))[:K].copy())


def oracle_decode(p, coder, norm_bbox):
    """CenterPointBBoxCoder.decode with the deterministic top-K (its arithmetic, on the head's device)."""
    heat = p["heatmap"].sigmoid()
    B, ncls, H, W = heat.shape
    K = min(coder.max_num, ncls * H * W)
    flat = heat.reshape(B, -1)
    idx = torch.stack([det_order(flat[b].float().cpu(), K) for b in range(B)]).to(heat.device)
    scores = flat.gather(1, idx)
    clses, cell = idx // (H * W), idx % (H * W)
    ys, xs = (cell // W).float(), (cell % W).float()
    pick = lambda t: t.reshape(B, t.shape[1], H * W).gather(2, cell[:, None].expand(-1, t.shape[1], -1)).transpose(1, 2)
    r = pick(p["reg"])
    xs, ys = xs + r[..., 0], ys + r[..., 1]
    dim = torch.exp(p["dim"]) if norm_bbox else p["dim"]
    rot = torch.atan2(pick(p["rot"][:, 0:1]), pick(p["rot"][:, 1:2]))
    xs = xs[..., None] * coder.out_size_factor * coder.voxel_size[0] + coder.pc_range[0]
    ys = ys[..., None] * coder.out_size_factor * coder.voxel_size[1] + coder.pc_range[1]
    parts = [xs, ys, pick(p["height"]), pick(dim), rot] + ([pick(p["vel"])] if "vel" in p else [])
    boxes = torch.cat(parts, dim=2)
    keep = torch.ones_like(scores, dtype=torch.bool) if coder.score_threshold is None else scores > coder.score_threshold
    if coder.post_center_range is not None:
        rng = boxes.new_tensor(coder.post_center_range)
        keep &= (boxes[..., :3] >= rng[:3]).all(2) & (boxes[..., :3] <= rng[3:]).all(2)
    return [(boxes[i, keep[i]].cpu(), scores[i, keep[i]].cpu(), clses[i, keep[i]].cpu()) for i in range(B)]


def _pairs_near(kind, bev, thr, post_max, margin=1e-4):
    """Whether a pair that the circle / size-aware greedy walk compares (a kept row against a later live one)
    lies within `margin` (relative) of deciding the other way."""
    bev = bev.astype(np.float32)
    n = len(bev)
    if kind != "circle":
        c, s = np.abs(np.cos(bev[:, 4])), np.abs(np.sin(bev[:, 4]))
        ex, ey = bev[:, 2] * c + bev[:, 3] * s, bev[:, 2] * s + bev[:, 3] * c
    alive, kept = np.ones(n, bool), 0
    for i in range(n):
        if not alive[i]:
            continue
        kept += 1
        if kept == post_max:
            break
        o = bev[i + 1:]
        if kind == "circle":
            d2 = ((o[:, :2] - bev[i, :2]) ** 2).sum(1)
            sup = d2 <= np.float32(thr)
            near = np.abs(d2 - np.float32(thr)) <= margin * max(abs(thr), 1e-6)
        else:
            hx, hy = (ex[i + 1:] + ex[i]) * thr / 2, (ey[i + 1:] + ey[i]) * thr / 2
            ax, ay = np.abs(o[:, 0] - bev[i, 0]), np.abs(o[:, 1] - bev[i, 1])
            cx, cy = ax <= hx, ay <= hy
            nx, ny = np.abs(ax - hx) <= margin * hx, np.abs(ay - hy) <= margin * hy
            sup = cx & cy
            near = (nx & (cy | ny)) | (ny & (cx | nx))
        if np.any(near & alive[i + 1:]):
            return True
        alive[i + 1:] &= ~sup
    return False


def oracle(preds, coder, test_cfg, num_classes, norm_bbox):
    """get_bboxes's [[bboxes, scores, labels], ...] (CPU) with the deterministic order, and whether a compared
    pair lay near its NMS threshold."""
    kind, P = test_cfg["nms_type"], test_cfg["post_max_size"]
    per_task, near = [], False
    for t, pd in enumerate(preds):
        rows = []
        for b3, sc, lb in oracle_decode(pd[0], coder, norm_bbox):
            if kind == "circle":
                dets = torch.cat([b3[:, :2], sc[:, None]], 1).numpy()
                keep = M.circle_nms(dets, test_cfg["min_radius"][t], P)
                near |= _pairs_near(kind, b3[:, [0, 1]].numpy(), test_cfg["min_radius"][t], P)
            elif kind == "size_aware_circle":
                dets = torch.cat([b3[:, [0, 1, 3, 4, 6]], sc[:, None]], 1).numpy()
                keep = M.size_aware_circle_nms(dets, test_cfg["thresh_scale"][t], P)
                near |= _pairs_near(kind, b3[:, [0, 1, 3, 4, 6]].numpy(), test_cfg["thresh_scale"][t], P)
            else:
                thr = test_cfg["nms_thr"][t] if isinstance(test_cfg["nms_thr"], (list, tuple)) else test_cfg["nms_thr"]
                keep, nr = rotate_nms(b3[:, [0, 1, 3, 4, 6]].numpy(), thr, test_cfg["pre_max_size"], P, margin=2e-4)
                near |= nr
            keep = torch.as_tensor(keep, dtype=torch.long)
            rows.append((b3[keep], sc[keep], lb[keep]))
        per_task.append(rows)
    out = []
    for i in range(len(per_task[0])):
        flag, labels = 0, []
        for t, n in enumerate(num_classes):
            labels.append(per_task[t][i][2].int() + flag)
            flag += n
        out.append([torch.cat([r[i][0] for r in per_task]), torch.cat([r[i][1] for r in per_task]),
                    torch.cat(labels)])
    return out, near


# ----------------------------------------------------------------------------- scenes
def head_setup(cfg, kind="circle", **test_kw):
    """(side, coder, test_cfg) of the reference head at the path configuration `cfg`."""
    _, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    side = hd["train_cfg"]["grid_size"][0] // 4
    coder = M.CenterPointBBoxCoder(**hd["bbox_coder"])
    tc = dict(hd["test_cfg"], nms_type=kind, thresh_scale=[1.0, 0.9, 1.1, 0.8, 1.0, 0.7])
    tc.update(test_kw)
    return side, coder, tc


def make_preds(B, H, W, scene, dtype, seed, dev, ncls=NCLS, has_vel=True):
    """Head outputs of one scene:
    dense   every logit above the threshold, boxes on every cell (worst case, heavy overlap);
    sparse  about 40 peaks per task on a -8 floor;
    below   every score under 0.1;
    ties    logits on a coarse lattice (large constant regions, ties at the K-th score);
    nan     dense with NaN logits sprinkled in;
    cluster the candidates packed into a 40 x 40-cell window (rotated NMS suppresses most of them)."""
    g = torch.Generator().manual_seed(seed)
    preds = []
    for n in ncls:
        shape = (B, n, H, W)
        if scene in ("dense", "nan"):
            heat = torch.randn(shape, generator=g) * 1.5 + 1.0
            if scene == "nan":
                heat[torch.rand(shape, generator=g) < 0.002] = float("nan")
        elif scene == "sparse":
            heat = torch.full(shape, -8.0)
            flat = heat.view(B, -1)
            for b in range(B):
                pos = torch.randint(0, n * H * W, (40,), generator=g)
                flat[b, pos] = torch.rand(40, generator=g) * 6 - 1
        elif scene == "cluster":
            heat = torch.full(shape, -8.0)
            y0, x0 = (H - min(H, 40)) // 2, (W - min(W, 40)) // 3
            win = heat[:, :, y0:y0 + 40, x0:x0 + 40]
            win.copy_(torch.randn(win.shape, generator=g) * 1.5 + 1.0)
        elif scene == "below":
            heat = torch.randn(shape, generator=g) * 0.3 - 4.0
        elif scene == "ties":
            heat = (torch.randn(shape, generator=g) * 2).round() / 2
        else:
            raise ValueError(scene)
        lo, hi = math.log(0.3), math.log(12.0)
        p = dict(heatmap=heat, reg=torch.rand(B, 2, H, W, generator=g),
                 height=torch.randn(B, 1, H, W, generator=g) * 2,
                 dim=torch.rand(B, 3, H, W, generator=g) * (hi - lo) + lo,
                 rot=torch.randn(B, 2, H, W, generator=g))
        if has_vel:
            p["vel"] = torch.randn(B, 2, H, W, generator=g) * 3
        preds.append([{k: v.to(dtype).to(dev) for k, v in p.items()}])
    return preds


def instance(B, H, W, scene, dtype, coder, tc, dev, seed=0, ncls=NCLS, has_vel=True, norm_bbox=True):
    """A scene that satisfies the margin rule (next seed otherwise) and its oracle output."""
    for s in range(seed, seed + 20):
        preds = make_preds(B, H, W, scene, dtype, s, dev, ncls=ncls, has_vel=has_vel)
        ref, near = oracle(preds, coder, tc, ncls, norm_bbox)
        if not near:
            return preds, ref
    pytest.fail("no instance outside the NMS margin in 20 seeds")


def assert_matches(res, ref, dtype, P, T):
    """Counts, labels, keep order and scores exact; x, y, height, vel bit-equal; dim and rot within one ulp of
    the head dtype; rows beyond the count zero."""
    boxes, scores, labels, counts = res.boxes.cpu(), res.scores.cpu(), res.labels.cpu(), res.counts.cpu()
    assert boxes.shape[:2] == (len(ref), T * P)
    for b, (rb, rs, rl) in enumerate(ref):
        n = int(counts[b])
        assert n == len(rl), (b, n, len(rl))
        assert torch.equal(labels[b, :n], rl), b
        assert torch.equal(scores[b, :n].view(BITS[dtype]), rs.view(BITS[dtype])), b
        cs = rb.shape[1]
        assert boxes.shape[2] == cs
        exact = [0, 1, 2] + ([7, 8] if cs == 9 else [])
        assert torch.equal(boxes[b, :n, exact].view(torch.int32), rb[:, exact].view(torch.int32)), b
        tol = rb[:, 3:7].abs() * EPS[dtype] + 1e-30
        assert ((boxes[b, :n, 3:7] - rb[:, 3:7]).abs() <= tol).all(), b
        assert not boxes[b, n:].any() and not labels[b, n:].any() and not scores[b, n:].float().any(), b


# ----------------------------------------------------------------------------- CPU: the oracle and the ABI
def test_rotated_iou_closed_forms():
    assert rotated_iou((1, 2, 3, 4, 0.3), (1, 2, 3, 4, 0.3)) == pytest.approx(1.0, abs=1e-12)
    assert rotated_iou((0, 0, 2, 2, 0.1), (10, 0, 2, 2, 1.0)) == 0.0
    # unit square against itself turned 45 degrees: octagon 2 (sqrt 2 - 1) over union 4 - 2 sqrt 2
    r2 = math.sqrt(2)
    assert rotated_iou((0, 0, 1, 1, 0), (0, 0, 1, 1, math.pi / 4)) == pytest.approx(
        2 * (r2 - 1) / (4 - 2 * r2), abs=1e-12)
    assert 2 * (r2 - 1) / (4 - 2 * r2) == pytest.approx(1 / r2, abs=1e-12)
    # contained: area ratio
    assert rotated_iou((0, 0, 4, 6, 0.7), (0.2, -0.3, 1, 2, 0.7)) == pytest.approx(2 / 24, abs=1e-12)
    # a 90 degree turn of dx x dy is the dy x dx box
    a = (0.5, -1.0, 2.0, 5.0, 0.0)
    for other in [(1.0, 0.0, 3.0, 1.5, 0.4), (0.0, 0.0, 1.0, 1.0, -1.2)]:
        assert rotated_iou((0.5, -1.0, 5.0, 2.0, math.pi / 2), other) == pytest.approx(rotated_iou(a, other), abs=1e-12)
    assert rotated_iou((0, 0, 0, 1, 0), (0, 0, 1, 1, 0)) == 0.0


def test_rotate_nms_oracle_greedy():
    bev = [(0, 0, 4, 2, 0), (0.5, 0, 4, 2, 0), (0, 0, 4, 2, math.pi / 2), (10, 0, 1, 1, 0)]
    # IoU(0, 1) = 3.5 / 4.5, IoU(0, 2) = 4 / 12
    assert rotate_nms(bev, 0.5, 10, 10)[0] == [0, 2, 3]
    assert rotate_nms(bev, 0.2, 10, 10)[0] == [0, 3]
    assert rotate_nms(bev, 0.5, 2, 10)[0] == [0]
    assert rotate_nms(bev, 0.5, 10, 2)[0] == [0, 2]


def test_det_order_is_total():
    v = torch.tensor([0.5, 0.7, float("nan"), 0.7, 0.1, float("nan"), 0.5])
    assert det_order(v, 7).tolist() == [2, 5, 1, 3, 0, 6, 4]
    assert det_order(v, 3).tolist() == [2, 5, 1]


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(**kw):
    d = _capi.VampDetDesc()
    d.B, d.T, d.H, d.W = 2, 6, 128, 128
    for t, n in enumerate(NCLS):
        d.ncls[t] = n
    d.max_num, d.pre_max_size, d.post_max_size = 500, 1000, 83
    d.nms_kind, d.in_dtype, d.has_vel, d.norm_bbox = _capi.VAMP_NMS_CIRCLE, _capi.VAMP_F32, 1, 1
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("field,value,message", [
    ("max_num", 1025, b"K = min(max_num"), ("T", 9, b"T must be in [1, 8]"), ("nms_kind", 3, b"unknown nms_kind"),
    ("post_max_size", 501, b"post_max_size must be in [1, max_num]"), ("in_dtype", 5, b"in_dtype must be"),
    ("B", 0, b"B must be"), ("T", 0, b"T must be in [1, 8]")])
def test_bad_descriptor_is_rejected_without_gpu(lib, field, value, message):
    """Every bad field returns VAMP_EINVAL with its message before any device work (all pointers are NULL: a
    call that went on would stop at the pointer checks instead); the valid descriptor stops there."""
    ok = _desc()
    assert lib.vamp_det_workspace_bytes(C.byref(ok)) > 0
    assert lib.vamp_det_postprocess(C.byref(ok), None, None, None, None, None, None, 0, None) == -1
    assert b"tasks is NULL" in lib.vamp_last_error()
    bad = _desc(**{field: value})
    assert lib.vamp_det_postprocess(C.byref(bad), None, None, None, None, None, None, 0, None) == -1
    assert message in lib.vamp_last_error(), lib.vamp_last_error()
    assert lib.vamp_det_workspace_bytes(C.byref(bad)) == 0


def test_bad_task_table_and_small_workspace_are_rejected(lib):
    d = _desc(T=1)
    table = (_capi.VampDetTask * 1)()
    assert lib.vamp_det_postprocess(C.byref(d), table, None, None, None, None, None, 0, None) == -1
    assert b"head pointer is NULL" in lib.vamp_last_error()
    d.ncls[0] = 5
    assert lib.vamp_det_postprocess(C.byref(d), table, None, None, None, None, None, 0, None) == -1
    assert b"ncls must be in [1, 4]" in lib.vamp_last_error()
    d.ncls[0], d.reserved = 1, 1
    assert lib.vamp_det_postprocess(C.byref(d), table, None, None, None, None, None, 0, None) == -1
    assert C.sizeof(_capi.VampDetDesc) == 58 * 4 and C.sizeof(_capi.VampDetTask) == 6 * 8


def test_cpu_tensors_are_refused():
    side, coder, tc = head_setup(CFG_TINY)
    preds = make_preds(1, 8, 8, "dense", torch.float32, 0, "cpu")
    with pytest.raises(_capi.VampireHipError):
        ops.det_postprocess(preds, coder, tc, NCLS, True)
    head = M.BEVDepthHead.__new__(M.BEVDepthHead)
    head.bbox_coder, head.test_cfg, head.num_classes, head.norm_bbox = coder, tc, NCLS, True
    with pytest.raises(_capi.VampireHipError):
        head.get_bboxes_device(preds)


# ----------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _identity_coder(max_num=1024):
    """x = column, y = row, no filter: every score of a 32 x 32 map comes back with its cell."""
    return M.CenterPointBBoxCoder(pc_range=[0.0, 0.0], out_size_factor=1, voxel_size=[1.0, 1.0],
                                  post_center_range=None, max_num=max_num, score_threshold=None)


def _all_scores(heat, dev):
    """Run a [B, T, 32, 32] heatmap (T tasks of one class) through det_postprocess with nothing filtered or
    suppressed; returns the scores placed back at their cells [B, T, 1024] and the NaN mask of the kernel's."""
    B, T = heat.shape[:2]
    z = torch.zeros(B, 2, 32, 32, dtype=heat.dtype, device=dev)
    preds = [[dict(heatmap=heat[:, t:t + 1].contiguous(), reg=z, height=z[:, :1], dim=torch.zeros(B, 3, 32, 32, dtype=heat.dtype, device=dev), rot=z)]
             for t in range(T)]
    tc = dict(nms_type="circle", min_radius=[-1.0] * T, post_max_size=1024)
    res = ops.det_postprocess(preds, _identity_coder(), tc, [1] * T, False)
    assert (res.counts == T * 1024).all()
    cell = (res.boxes[..., 1].long() * 32 + res.boxes[..., 0].long()).view(B, T, 1024)
    task = (res.labels.long()).view(B, T, 1024)
    assert torch.equal(task, torch.arange(T, device=dev)[None, :, None].expand(B, T, 1024))
    assert torch.equal(cell.sort(2).values, torch.arange(1024, device=dev).expand(B, T, 1024))
    sc = res.scores.view(B, T, 1024)
    # order: NaN first, then score descending, ties by cell ascending
    f = sc.float()
    key = torch.where(f.isnan(), torch.full_like(f, float("inf")), f)
    assert (key[..., :-1] >= key[..., 1:]).all()
    tie = key[..., :-1] == key[..., 1:]
    assert (cell[..., :-1][tie] < cell[..., 1:][tie]).all()
    placed = torch.empty_like(sc).scatter_(2, cell, sc)
    return placed


@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_scores_bit_exact_all_16bit_patterns(dev, dtype):
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    heat = bits.view(dtype).reshape(8, 8, 32, 32).to(dev)
    got = _all_scores(heat, dev).view(8, 8, 32, 32)
    want = torch.sigmoid(heat)
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))


@gpu
def test_scores_bit_exact_fp32(dev):
    g = torch.Generator().manual_seed(7)
    n = 1 << 24
    x = torch.randint(-(1 << 31), 1 << 31, (n,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    x[: n // 2] = torch.randn(n // 2, generator=g) * 12                 # the range where sigmoid is not 0 or 1
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 88.0, -88.0, 88.7, -88.7,
                            103.9, -103.9, float("inf"), float("-inf"), float("nan"), 17.0, -17.0])
    x[: len(special)] = special
    chunk = 512 * 8 * 1024
    for c in range(0, n, chunk):
        heat = x[c:c + chunk].reshape(512, 8, 32, 32).to(dev)
        got = _all_scores(heat, dev).view(512, 8, 32, 32)
        want = torch.sigmoid(heat)
        nan = want.isnan()
        assert torch.equal(got.isnan(), nan)
        assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32)), c


CASES = [("A", "dense"), ("A", "sparse"), ("B", "dense"), ("B", "ties"), ("A", "nan"), ("A", "below")]


@gpu
@pytest.mark.parametrize("kind", ["circle", "size_aware_circle"])
@pytest.mark.parametrize("cfg,scene", CASES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_against_deterministic_oracle(dev, kind, cfg, scene, dtype):
    side, coder, tc = head_setup({"A": CFG_A, "B": CFG_B}[cfg], kind)
    B = {"dense": 3, "sparse": 8, "ties": 1, "nan": 3, "below": 8}[scene]
    preds, ref = instance(B, side, side, scene, dtype, coder, tc, dev)
    res = ops.det_postprocess(preds, coder, tc, NCLS, True)
    assert_matches(res, ref, dtype, tc["post_max_size"], len(NCLS))
    counts = res.counts.cpu()
    if scene == "below":
        assert not counts.any()
    if scene == "dense" and kind == "circle":
        assert (counts > 83).all()           # the small-radius tasks hit post_max_size
    if scene in ("dense", "ties", "nan"):
        assert counts.min() > 0


@gpu
@pytest.mark.parametrize("kind", ["circle", "size_aware_circle", "rotate"])
def test_tiny_grid_and_truncation(dev, kind):
    """K = ncls * H * W below max_num (a 4 x 5 grid), no velocity, dims not normalised; then post_max_size 7."""
    _, coder, tc = head_setup(CFG_TINY, kind, min_radius=[0.5] * 6)
    preds, ref = instance(3, 4, 5, "dense", torch.float32, coder, tc, dev, has_vel=False, norm_bbox=False)
    assert_matches(ops.det_postprocess(preds, coder, tc, NCLS, False), ref, torch.float32, 83, 6)
    tc = dict(tc, post_max_size=7)
    preds, ref = instance(2, 4, 5, "dense", torch.bfloat16, coder, tc, dev, seed=3)
    res = ops.det_postprocess(preds, coder, tc, NCLS, True)
    assert_matches(res, ref, torch.bfloat16, 7, 6)


@gpu
@pytest.mark.parametrize("cfg,B,pre", [("A", 1, 1000), ("A", 3, 150), ("B", 2, 1000)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rotate_against_float64_oracle(dev, cfg, B, pre, dtype):
    """Dense overlapping scenes, random yaw, sizes 0.3 m to 12 m; pre_max_size 150 < K = 500 in one case."""
    side, coder, tc = head_setup({"A": CFG_A, "B": CFG_B}[cfg], "rotate", pre_max_size=pre, nms_thr=0.2)
    preds, ref = instance(B, side, side, "cluster", dtype, coder, tc, dev, seed=B)
    res = ops.det_postprocess(preds, coder, tc, NCLS, True)
    assert_matches(res, ref, dtype, tc["post_max_size"], 6)
    assert (res.counts > 6 * 10).all()


def _graph_out(B, P, T, dtype, dev, cs=9):
    return ops.DetResult(torch.empty(B, T * P, cs, device=dev), torch.empty(B, T * P, dtype=dtype, device=dev),
                         torch.empty(B, T * P, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))


@gpu
@pytest.mark.parametrize("kind", ["circle", "rotate"])
def test_no_sync_and_graph_replay(dev, kind):
    side, coder, tc = head_setup(CFG_A, kind)
    preds = make_preds(2, side, side, "dense", torch.bfloat16, 1, dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = ops.det_postprocess(preds, coder, tc, NCLS, True)
        out = _graph_out(2, 83, 6, torch.bfloat16, dev)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.det_postprocess(preds, coder, tc, NCLS, True, out=out)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.det_postprocess(preds, coder, tc, NCLS, True, out=out)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    for seed in (5, 6, 7):
        fresh = make_preds(2, side, side, "dense" if seed != 6 else "sparse", torch.bfloat16, seed, dev)
        for pd, fd in zip(preds, fresh):
            for k in pd[0]:
                pd[0][k].copy_(fd[0][k])
        g.replay()
        eager = ops.det_postprocess(preds, coder, tc, NCLS, True)
        torch.cuda.synchronize()
        for a, b in zip(dataclasses.astuple(out), dataclasses.astuple(eager)):
            assert torch.equal(a, b), seed


@gpu
def test_against_get_bboxes_distinct_scores(dev):
    """The untouched host get_bboxes on fp32 heads whose scores are pairwise distinct (torch.topk's order of ties
    cannot matter): to_list() equals it."""
    side, coder, tc = head_setup(CFG_A)
    head = M.BEVDepthHead.__new__(M.BEVDepthHead)
    head.bbox_coder, head.num_classes, head.norm_bbox = coder, NCLS, True
    for kind in ("circle", "size_aware_circle"):
        head.test_cfg = dict(tc, nms_type=kind)
        for seed in range(10, 30):
            preds = make_preds(3, side, side, "dense", torch.float32, seed, dev)
            for pd in preds:                     # distinct logits -> distinct scores near the top
                h = pd[0]["heatmap"]
                perm = torch.randperm(h.numel(), generator=torch.Generator().manual_seed(seed)).view_as(h)
                h.copy_(perm.to(dev) * (4.0 / h.numel()) - 2.0)
            ref, near = oracle(preds, coder, head.test_cfg, NCLS, True)
            if not near:
                break
        host = head.get_bboxes(preds)
        dev_list = head.get_bboxes_device(preds).to_list()
        for (hb, hs, hl), (db, ds, dl), (rb, rs, rl) in zip(host, dev_list, ref):
            assert torch.equal(hl.cpu(), dl.cpu()) and torch.equal(hs.cpu(), ds.cpu())
            assert torch.equal(hb[:, [0, 1, 2, 7, 8]].cpu(), db[:, [0, 1, 2, 7, 8]].cpu())
            assert ((hb[:, 3:7] - db[:, 3:7]).abs() <= hb[:, 3:7].abs() * EPS[torch.float32]).all()
            assert torch.equal(rl, dl.cpu())


def _tiny_model(cfg, dev):
    torch.manual_seed(0)
    bb, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(cfg.sdf_bias)
    return model


@gpu
@pytest.mark.parametrize("amp", [None, torch.bfloat16])
@pytest.mark.parametrize("kind", ["circle", "size_aware_circle", "rotate"])
def test_end_to_end_small_model(dev, amp, kind):
    cfg = dataclasses.replace(CFG_TINY, density_mode="sdf", final_dim=(192, 224), num_classes=6)
    model = _tiny_model(cfg, dev).eval()
    model.head.test_cfg = dict(model.head.test_cfg, nms_type=kind, thresh_scale=[1.0] * 6)
    batch = M.synthetic_batch(cfg, 2, seed=5, device=dev, num_points=40, num_boxes=6)
    with torch.no_grad(), torch.autocast("cuda", dtype=amp or torch.float32, enabled=amp is not None):
        out = model(batch[0], batch[1], inrange_pts=batch[11])
        preds = out[0]
        for pd in preds:                         # lift a few cells above the threshold
            pd[0]["heatmap"].view(-1)[::7] += 3.0
        got = model.get_bboxes_device(preds).to_list()
    ref, _ = oracle(preds, model.head.bbox_coder, model.head.test_cfg, model.head.num_classes, True)
    dtype = preds[0][0]["heatmap"].dtype
    assert sum(len(r[2]) for r in ref) > 0
    for (gb, gs, gl), (rb, rs, rl) in zip(got, ref):
        assert torch.equal(gl.cpu(), rl) and torch.equal(gs.cpu().view(BITS[dtype]), rs.view(BITS[dtype]))
        assert torch.equal(gb[:, [0, 1, 2, 7, 8]].cpu(), rb[:, [0, 1, 2, 7, 8]])
        assert ((gb[:, 3:7].cpu() - rb[:, 3:7]).abs() <= rb[:, 3:7].abs() * EPS[dtype]).all()
    if kind == "circle":
        flat = torch.cat([pd[0]["heatmap"].sigmoid().flatten() for pd in preds])
        if flat.unique().numel() == flat.numel():
            host = model.get_bboxes(preds)
            for (hb, hs, hl), (gb, gs, gl) in zip(host, got):
                assert torch.equal(hl, gl) and torch.equal(hs, gs)
