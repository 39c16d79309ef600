"""Detection training targets on the device (ops.det_targets / BEVDepthHead.get_targets_device over the HIP
kernels of det_targets.hip) against an oracle that replays the reference's get_targets (bev_depth_head.py:168-319)
box by box with torch ops on 0-dim tensors of the GPU -- so that torch itself supplies the reference's fp32
rounding, its division by CPU scalars included -- and builds the Gaussian stamps in float64 with numpy, as
mmdet3d does.  The oracle departs from the reference in one place: a box whose radius is not finite makes the
reference raise (int(nan)); the oracle skips it, as the device path does.

Exactness: heatmaps, inds and masks are compared with torch.equal, anno bit for bit (NaN against NaN allowed).
Against the untouched host get_targets, which computes centres and radii in float64 Python floats and its stamps
in fp32, the comparison carries the tolerances stated at each test."""
import ctypes as C
import dataclasses
import functools
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
CFGS = {"A": CFG_A, "B": CFG_B}


def train_cfg(cfg, **kw):
    tc = dict(M.reference_confs(cfg, output_channels=8, small_encoder=True)[1]["train_cfg"])
    tc.update(kw)
    return tc


# ----------------------------------------------------------------------------- the oracle
@functools.lru_cache(maxsize=None)
def stamp64(r):
    """mmdet3d's Gaussian for radius r: side 2r + 1, sigma = side / 6, float64, tiny values cut to zero."""
    side = 2 * r + 1
    sigma = side / 6
    half = (side - 1.0) / 2.0
    ys, xs = np.ogrid[-half:half + 1, -half:half + 1]
    g = np.exp(-(xs * xs + ys * ys) / (2 * sigma * sigma))
    g[g < np.finfo(g.dtype).eps * g.max()] = 0
    return g


def paint(plane, x, y, r):
    """Max-merge the stamp into plane [fh, fw] at (x, y), clipped to the map."""
    fh, fw = plane.shape
    lo_x, hi_x = min(x, r), min(fw - x, r + 1)
    lo_y, hi_y = min(y, r), min(fh - y, r + 1)
    win = plane[y - lo_y:y + hi_y, x - lo_x:x + hi_x]
    g = torch.from_numpy(stamp64(r)[r - lo_y:r + hi_y, r - lo_x:r + hi_x]).to(plane.device, torch.float32)
    if min(win.shape) > 0 and min(g.shape) > 0:
        torch.maximum(win, g, out=win)


def radius_of(h, w, o):
    """The CornerNet radius on 0-dim device tensors, in the reference's operation order."""
    s1 = h + w
    p1 = w * h * (1 - o) / (1 + o)
    root1 = (s1 + torch.sqrt(s1 ** 2 - 4 * 1 * p1)) / 2
    s2 = 2 * (h + w)
    p2 = (1 - o) * w * h
    root2 = (s2 + torch.sqrt(s2 ** 2 - 4 * 4 * p2)) / 2
    q3 = 4 * o
    s3 = -2 * o * (h + w)
    p3 = (o - 1) * w * h
    root3 = (s3 + torch.sqrt(s3 ** 2 - 4 * q3 * p3)) / 2
    return min(root1, root2, root3)


def oracle_sample(boxes, labels, ncls, tc, norm_bbox):
    """get_targets_single of one sample (boxes [n, 7 | 9] fp32, labels [n], both on the GPU)."""
    dev = boxes.device
    limit = tc["max_objs"] * tc["dense_reg"]
    osf = tc["out_size_factor"]
    vsz = torch.tensor(tc["voxel_size"])
    pcr = torch.tensor(tc["point_cloud_range"])
    fmap = torch.tensor(tc["grid_size"])[:2] // osf
    fw, fh = int(fmap[0]), int(fmap[1])
    width = len(tc["code_weights"])
    out = ([], [], [], [])
    base = 0
    for n in ncls:
        picks = [torch.where(labels == base + c)[0] for c in range(n)]
        tb = torch.cat([boxes[i] for i in picks], 0)
        tcls = torch.cat([torch.full((len(i),), c, dtype=torch.long) for c, i in enumerate(picks)])
        base += n
        heat = torch.zeros(n, fh, fw, device=dev)
        anno = torch.zeros(limit, width, device=dev)
        ind = torch.zeros(limit, dtype=torch.int64, device=dev)
        msk = torch.zeros(limit, dtype=torch.uint8, device=dev)
        for k in range(min(len(tb), limit)):
            box = tb[k]
            sx = box[3] / vsz[0] / osf
            sy = box[4] / vsz[1] / osf
            if not (sx > 0 and sy > 0):
                continue
            rad = radius_of(sy, sx, tc["gaussian_overlap"])
            if not torch.isfinite(rad):           # the reference raises here; the device path skips the box
                continue
            r = max(tc["min_radius"], int(rad))
            cx = (box[0] - pcr[0]) / vsz[0] / osf
            cy = (box[1] - pcr[1]) / vsz[1] / osf
            centre = torch.stack([cx, cy])
            cell = centre.to(torch.int32)
            x, y = int(cell[0]), int(cell[1])
            if not (0 <= x < fw and 0 <= y < fh):
                continue
            paint(heat[int(tcls[k])], x, y, r)
            ind[k] = y * fw + x
            msk[k] = 1
            dims = box[3:6].log() if norm_bbox else box[3:6]
            row = [centre - cell, box[2:3], dims, box[6:7].sin(), box[6:7].cos()]
            if box.shape[0] > 7:
                row.append(box[7:9])
            anno[k] = torch.cat(row)
        for lst, v in zip(out, (heat, anno, ind, msk)):
            lst.append(v)
    return out


def oracle(boxes, labels, ncls, tc, norm_bbox):
    per = [oracle_sample(b, l, ncls, tc, norm_bbox) for b, l in zip(boxes, labels)]
    return tuple([torch.stack([p[j][t] for p in per]) for t in range(len(ncls))] for j in range(4))


# ----------------------------------------------------------------------------- comparisons
def same_bits(a, b):
    """Bitwise equality of fp32 tensors, any NaN matching any NaN."""
    if a.shape != b.shape:
        return False
    both_nan = a.isnan() & b.isnan()
    return bool(((a.view(torch.int32) == b.view(torch.int32)) | both_nan).all())


def assert_matches_oracle(got, ref):
    heat, anno, inds, masks = got.as_tuple()
    rh, ra, ri, rm = ref
    for t in range(len(rh)):
        assert torch.equal(inds[t], ri[t]), f"task {t}: inds"
        assert torch.equal(masks[t], rm[t]), f"task {t}: masks"
        assert same_bits(anno[t], ra[t]), f"task {t}: anno, columns {anno_diff_columns(anno[t], ra[t])}"
        assert torch.equal(heat[t], rh[t]), f"task {t}: heatmap, {int((heat[t] != rh[t]).sum())} pixels differ"


def anno_diff_columns(a, b):
    bad = (a.view(torch.int32) != b.view(torch.int32)) & ~(a.isnan() & b.isnan())
    return sorted(set(torch.nonzero(bad)[:, -1].tolist()))


def ulps(a, b):
    """|a - b| in units of the last place of b (fp32), elementwise."""
    ia, ib = a.view(torch.int32).long(), b.view(torch.int32).long()
    ia = torch.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = torch.where(ib < 0, -(ib & 0x7fffffff), ib)
    return (ia - ib).abs()


# ----------------------------------------------------------------------------- scenes
def random_scene(B, n, cfg, seed, cols=9, label_dtype=torch.int64, dev="cpu"):
    """n boxes per sample over the detection range and a margin around it; for n >= 100 most boxes are cars
    (task 0), so that a task holds more than max_objs = 500 boxes."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = cfg.x_bound_det[0], cfg.x_bound_det[1]
    boxes, labels = [], []
    for _ in range(B):
        xy = torch.rand(n, 2, generator=g) * (hi - lo) * 1.1 + lo * 1.1
        z = torch.rand(n, 1, generator=g) * 3 - 2
        dims = torch.rand(n, 3, generator=g) * torch.tensor([6.0, 12.0, 3.0]) + 0.2
        yaw = (torch.rand(n, 1, generator=g) * 2 - 1) * math.pi
        vel = torch.randn(n, 2, generator=g)
        b = torch.cat([xy, z, dims, yaw, vel], 1)[:, :cols].contiguous()
        lab = torch.randint(0, 10, (n,), generator=g)
        if n >= 100:
            lab = torch.where(torch.rand(n, generator=g) < 0.9, torch.zeros_like(lab), lab)
        boxes.append(b.to(dev))
        labels.append(lab.to(label_dtype).to(dev))
    return boxes, labels


def edge_scene(cfg, cols=9):
    """One sample of hand-made boxes: boundary centres, out-of-range and NaN centres, bad sizes, foreign labels,
    shared cells, overlapping stamps, radii beyond the map."""
    pc0, pc1 = cfg.x_bound_det[0], cfg.y_bound_det[0]
    cell = (cfg.x_bound_det[1] - cfg.x_bound_det[0]) / (cfg.oY // 2 if cfg.oY == 256 else cfg.oY)
    nan, inf = float("nan"), float("inf")
    f32 = lambda v: float(np.float32(v))
    rows = []                    # (x, y, dx, dy, label)
    for k in range(0, 129, 7):   # centres on cell boundaries, as fp32
        rows.append((f32(pc0 + k * cell), f32(pc1 + (k * 3 % 120) * cell), 1.9, 4.5, k % 10))
    rows += [(pc0, pc1, 2.0, 4.0, 0), (pc0 - 0.3 * cell, pc1 + 5.5 * cell, 2.0, 4.0, 1),
             (pc0 + 3.5 * cell, pc1 - 0.7 * cell, 2.0, 4.0, 2), (-pc0, 0.0, 2.0, 4.0, 3),
             (f32(-pc0 - 1e-3), f32(-pc1 - 1e-3), 2.0, 4.0, 4), (-pc0 + 2.0, 0.0, 2.0, 4.0, 5),
             (0.0, 0.0, 0.0, 4.0, 0), (0.0, 0.0, -1.0, 4.0, 0), (1.0, 1.0, nan, 4.0, 0), (1.0, 1.0, 2.0, nan, 0),
             (nan, 3.0, 2.0, 4.0, 0), (3.0, nan, 2.0, 4.0, 8), (nan, nan, 1.0, 1.0, 9), (2.0, 2.0, inf, 4.0, 0),
             (5.0, 5.0, 2.0, 4.0, -1), (5.0, 5.0, 2.0, 4.0, 10), (5.0, 5.0, 2.0, 4.0, 99),
             (10.1, 10.1, 2.0, 4.0, 0), (10.2, 10.15, 3.0, 5.0, 0), (10.3, 10.2, 0.5, 0.5, 0),
             (12.0, 12.0, 8.0, 10.0, 0), (13.5, 11.0, 1.0, 2.0, 0), (14.0, 14.0, 20.0, 30.0, 0),
             (0.0, 0.0, 300.0, 200.0, 6), (20.0, -20.0, 900.0, 900.0, 7), (21.0, -20.0, 1e-4, 1e-4, 7)]
    n = len(rows)
    t = torch.tensor([[r[0], r[1]] for r in rows], dtype=torch.float32)
    z = torch.linspace(-2, 1, n)[:, None]
    dims = torch.tensor([[r[2], r[3], 1.5] for r in rows], dtype=torch.float32)
    yaw = torch.linspace(-3.1, 3.1, n)[:, None]
    vel = torch.stack([torch.linspace(-1, 1, n), torch.linspace(2, -2, n)], 1)
    boxes = torch.cat([t, z, dims, yaw, vel], 1)[:, :cols].contiguous()
    labels = torch.tensor([r[4] for r in rows])
    return boxes, labels


# ----------------------------------------------------------------------------- CPU: the C ABI boundary
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(**kw):
    d = _capi.VampDetTargetDesc()
    d.gaussian_overlap = 0.1
    d.B, d.T, d.M = 2, 6, 40
    for t, n in enumerate(NCLS):
        d.ncls[t] = n
    d.box_cols, d.code, d.max_objs, d.fh, d.fw = 9, 10, 500, 128, 128
    d.out_size_factor, d.min_radius, d.norm_bbox, d.label_dtype = 4, 2, 1, _capi.VAMP_I64
    d.voxel_size[0], d.voxel_size[1] = 0.2, 0.2
    d.pc_range[0], d.pc_range[1] = -51.2, -51.2
    for k, v in kw.items():
        if callable(v):
            v(d)
        else:
            setattr(d, k, v)
    return d


def _set(field, i, v):
    def f(d):
        getattr(d, field)[i] = v
    return f


BAD = [("T", 0, b"T must be in [1, 8]"), ("T", 9, b"T must be in [1, 8]"),
       ("ncls", _set("ncls", 2, 5), b"ncls must be in [1, 4]"), ("ncls", _set("ncls", 0, 0), b"ncls must be in [1, 4]"),
       ("max_objs", 0, b"max_objs must be in"), ("max_objs", -3, b"max_objs must be in"),
       ("max_objs", 8193, b"max_objs must be in"), ("code", 9, b"code must be 8 or 10"),
       ("code", 8, b"code must be box_cols + 1"), ("box_cols", 7, b"code must be box_cols + 1"),
       ("box_cols", 8, b"box_cols must be 7 or 9"), ("fh", 0, b"fh, fw must be in"), ("fw", -1, b"fh, fw must be in"),
       ("fw", 8193, b"fh, fw must be in"), ("out_size_factor", 0, b"out_size_factor must be positive"),
       ("voxel", _set("voxel_size", 0, 0.0), b"voxel_size must be positive"),
       ("voxel", _set("voxel_size", 1, -0.2), b"voxel_size must be positive"),
       ("voxel", _set("voxel_size", 0, float("nan")), b"voxel_size must be positive"),
       ("B", 0, b"B must be in"), ("M", -1, b"M must be in"), ("label_dtype", _capi.VAMP_F32, b"label_dtype must be"),
       ("reserved", _set("reserved", 1, 1), b"reserved must be 0")]


@pytest.mark.parametrize("field,value,message", BAD, ids=[f"{b[0]}-{i}" for i, b in enumerate(BAD)])
def test_bad_descriptor_is_rejected_without_gpu(lib, field, value, message):
    """Every bad field returns VAMP_EINVAL with its message before any device work (all pointers are NULL: a
    call that went on would stop at the pointer checks instead); the valid descriptor stops there."""
    ok = _desc()
    assert lib.vamp_det_targets_workspace_bytes(C.byref(ok)) > 0
    assert lib.vamp_det_targets(C.byref(ok), None, None, None, None, None, None, None, 0, None) == -1
    assert b"boxes or labels is NULL" in lib.vamp_last_error()
    bad = _desc(**{field: value})
    assert lib.vamp_det_targets(C.byref(bad), None, None, None, None, None, None, None, 0, None) == -1
    assert message in lib.vamp_last_error(), lib.vamp_last_error()
    assert lib.vamp_det_targets_workspace_bytes(C.byref(bad)) == 0


def test_small_workspace_and_null_outputs_are_rejected(lib):
    """A workspace one byte short returns VAMP_ENOSPC before any launch (the pointers are never dereferenced)."""
    d = _desc()
    need = lib.vamp_det_targets_workspace_bytes(C.byref(d))
    fake = [C.c_void_p(256 * (i + 1)) for i in range(7)]
    assert lib.vamp_det_targets(C.byref(d), fake[0], fake[1], None, fake[3], fake[4], fake[5], fake[6], need,
                                None) == -1
    assert b"an output pointer is NULL" in lib.vamp_last_error()
    assert lib.vamp_det_targets(C.byref(d), *fake, need - 1, None) == -2
    assert b"workspace" in lib.vamp_last_error()
    assert lib.vamp_det_targets(C.byref(d), *fake[:6], None, need, None) == -2
    d.M = 0                      # no boxes: the box and label pointers may be NULL
    assert lib.vamp_det_targets(C.byref(d), None, None, fake[2], fake[3], fake[4], fake[5], fake[6], 0, None) == -2
    assert C.sizeof(_capi.VampDetTargetDesc) == 112


def test_cpu_tensors_and_wrong_dtypes_are_refused():
    tc = train_cfg(CFG_A)
    boxes, labels = random_scene(2, 5, CFG_A, 0)
    with pytest.raises(_capi.VampireHipError):
        ops.det_targets(boxes, labels, NCLS, tc, True)
    with pytest.raises(_capi.VampireHipError):
        ops.det_targets(torch.stack(boxes), torch.stack(labels), NCLS, tc, True)
    with pytest.raises(TypeError):
        ops.det_targets([b.double() for b in boxes], labels, NCLS, tc, True)
    with pytest.raises(TypeError):
        ops.det_targets(torch.stack(boxes).half(), torch.stack(labels), NCLS, tc, True)
    with pytest.raises(TypeError):
        ops.det_targets(torch.stack(boxes), torch.stack(labels).float(), NCLS, tc, True)
    head = M.BEVDepthHead(**M.reference_confs(CFG_TINY, output_channels=8, small_encoder=True)[1])
    with pytest.raises(_capi.VampireHipError):
        head.get_targets_device(boxes, labels)
    with pytest.raises(ValueError):
        M.MultiTaskLoss(head, det_targets="gpu")
    assert M.MultiTaskLoss(head).det_targets == "host"


# ----------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@gpu
def test_torch_divides_by_a_cpu_scalar_through_its_reciprocal(dev):
    """What the kernels assume of aten on this device: a device tensor over a CPU scalar is a product with the
    scalar's reciprocal, not a correctly rounded quotient -- 1.0f / b in fp32 for a 0-dim fp32 tensor (the
    reference's voxel_size[i]), (float) (1.0 / b) for a Python float (its 1 + gaussian_overlap)."""
    x = torch.rand(1 << 16, generator=torch.Generator().manual_seed(0)) * 200 - 100
    xd = x.to(dev)
    for b in (0.2, 0.1, 1.1, 0.8, 1.7):
        by_tensor = torch.from_numpy(x.numpy() * (np.float32(1.0) / np.float32(b)))
        by_number = torch.from_numpy(x.numpy() * np.float32(1.0 / b))
        assert torch.equal((xd / torch.tensor(b)).cpu(), by_tensor)
        assert torch.equal((xd / b).cpu(), by_number)
        assert not torch.equal(by_tensor, x / torch.tensor(b))     # the true quotient differs somewhere
    assert not torch.equal((xd / 1.1).cpu(), (xd / torch.tensor(1.1)).cpu())


@gpu
@pytest.mark.parametrize("n", [0, 1, 40, 600])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_against_oracle(dev, cfg, B, n):
    c = CFGS[cfg]
    tc = train_cfg(c)
    boxes, labels = random_scene(B, n, c, 100 * B + n, dev=dev)
    got = ops.det_targets(boxes, labels, NCLS, tc, True)
    ref = oracle(boxes, labels, NCLS, tc, True)
    assert_matches_oracle(got, ref)
    if n == 600:                                  # task 0 was truncated to max_objs
        assert bool((ref[3][0].sum(1) > 0).all()) and len(torch.where(labels[0] == 0)[0]) > tc["max_objs"]
    if n:
        assert int(sum(m.sum() for m in ref[3])) > 0


@gpu
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_truncation_within_a_task(dev, cfg):
    c = CFGS[cfg]
    tc = train_cfg(c, max_objs=5)
    boxes, labels = random_scene(3, 40, c, 7, dev=dev)
    for lab in labels:                            # task 1 (labels 1, 2) holds more than 5 boxes of both classes
        lab[::3] = 2
        lab[1::3] = 1
    got = ops.det_targets(boxes, labels, NCLS, tc, True)
    assert_matches_oracle(got, oracle(boxes, labels, NCLS, tc, True))


@gpu
@pytest.mark.parametrize("label_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("norm_bbox", [True, False])
@pytest.mark.parametrize("cols", [9, 7])
@pytest.mark.parametrize("cfg", ["A", "B"])
def test_edge_cases(dev, cfg, cols, norm_bbox, label_dtype):
    c = CFGS[cfg]
    tc = train_cfg(c)
    if cols == 7:
        tc["code_weights"] = tc["code_weights"][:8]
    b0, l0 = edge_scene(c, cols)
    b1, l1 = random_scene(1, 30, c, 3, cols=cols)
    boxes = [b0.to(dev), b1[0].to(dev)]
    labels = [l0.to(label_dtype).to(dev), l1[0].to(label_dtype).to(dev)]
    got = ops.det_targets(boxes, labels, NCLS, tc, norm_bbox)
    ref = oracle(boxes, labels, NCLS, tc, norm_bbox)
    assert_matches_oracle(got, ref)
    assert got.anno.shape[-1] == cols + 1
    # the NaN-x centre lands in column 0 of the map, as torch's cast puts it there
    heat, anno, inds, masks = got.as_tuple()
    assert bool(anno[0][0].isnan().any())


@gpu
def test_repeatable_and_fully_overwritten(dev):
    tc = train_cfg(CFG_A)
    boxes, labels = random_scene(3, 40, CFG_A, 11, dev=dev)
    a = ops.det_targets(boxes, labels, NCLS, tc, True)
    b = ops.det_targets(boxes, labels, NCLS, tc, True)
    fill = ops.det_targets(boxes, labels, NCLS, tc, True)
    fill.heat.fill_(float("nan"))
    fill.anno.fill_(float("nan"))
    fill.inds.fill_(-1)
    fill.masks.fill_(0xFF)
    c = ops.det_targets(boxes, labels, NCLS, tc, True, out=fill)
    assert c is fill
    for x, y, z in zip((a.heat, a.anno, a.inds, a.masks), (b.heat, b.anno, b.inds, b.masks),
                       (c.heat, c.anno, c.inds, c.masks)):
        assert torch.equal(x, y) and torch.equal(x, z)


@gpu
def test_no_sync_and_graph_replay(dev):
    tc = train_cfg(CFG_A)
    boxes, labels = random_scene(4, 40, CFG_A, 21, dev=dev)
    packed_b = torch.nn.utils.rnn.pad_sequence(boxes, batch_first=True)
    packed_l = torch.nn.utils.rnn.pad_sequence(labels, batch_first=True, padding_value=-1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = ops.det_targets(boxes, labels, NCLS, tc, True)
        out = ops.det_targets(packed_b, packed_l, NCLS, tc, True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.det_targets(packed_b, packed_l, NCLS, tc, True, out=out)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.det_targets(packed_b, packed_l, NCLS, tc, True, out=out)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    for x, y in zip((eager.heat, eager.anno, eager.inds, eager.masks), (out.heat, out.anno, out.inds, out.masks)):
        assert torch.equal(x, y)
    for seed in (5, 6, 7):
        fb, fl = random_scene(4, 40, CFG_A, seed, dev=dev)
        packed_b.copy_(torch.stack(fb))
        packed_l.copy_(torch.stack(fl))
        g.replay()
        ref = ops.det_targets(packed_b, packed_l, NCLS, tc, True)
        torch.cuda.synchronize()
        for x, y in zip((ref.heat, ref.anno, ref.inds, ref.masks), (out.heat, out.anno, out.inds, out.masks)):
            assert torch.equal(x, y), seed
        assert int(out.masks.sum()) > 0


# ----------------------------------------------------------------------------- GPU: the host get_targets
def _head(cfg):
    torch.manual_seed(0)
    return M.BEVDepthHead(**M.reference_confs(cfg, output_channels=8, small_encoder=True)[1])


@gpu
@pytest.mark.parametrize("num_boxes", [12, 40])
@pytest.mark.parametrize("seed", [0, 1])
def test_against_host_get_targets(dev, seed, num_boxes):
    """inds and masks equal the host's.  The host computes the centre in float64 and rounds the offset to fp32,
    the device rounds every step of the fp32 chain: the regression offsets agree to 4 ulps of the map width.
    Copied columns (z, velocity) are equal; log / sin / cos, which the host computes on the CPU, agree to 2 ulps.  The host's fp32 stamps are up to 6 ulps from mmdet3d's float64 ones: heatmaps agree to
    8 ulps."""
    batch = M.synthetic_batch(CFG_A, 8, seed=seed, device=dev, num_points=10, num_boxes=num_boxes)
    head = _head(CFG_A).to(dev)
    host = head.get_targets(batch[4], batch[5])
    got = head.get_targets_device(batch[4], batch[5]).as_tuple()
    fw = head.train_cfg["grid_size"][0] // head.train_cfg["out_size_factor"]
    for t in range(len(NCLS)):
        assert torch.equal(got[2][t], host[2][t]) and torch.equal(got[3][t], host[3][t])
        ga, ha = got[1][t], host[1][t]
        assert torch.equal(ga[..., [2, 8, 9]], ha[..., [2, 8, 9]])
        assert float((ga[..., :2] - ha[..., :2]).abs().max()) <= 4 * fw * 2.0 ** -24
        assert int(ulps(ga[..., 3:8], ha[..., 3:8]).max()) <= 2
        assert int(ulps(got[0][t], host[0][t]).max()) <= 8
        assert bool((got[0][t] == 1).sum() == (host[0][t] == 1).sum())


@gpu
def test_boundary_centre_host_one_cell_low(dev):
    """x = pc_range[0] + k * cell as fp32: the host's float64 chain puts some of these in cell k - 1, the fp32
    chain (the reference's, the oracle's and the device's) in cell k."""
    head = _head(CFG_A)
    tc = head.train_cfg
    pc0, vs, osf = tc["point_cloud_range"][0], tc["voxel_size"][0], tc["out_size_factor"]
    inv_vs, inv_osf = np.float32(1) / np.float32(vs), np.float32(1) / np.float32(osf)
    for k in range(1, 128):
        x = np.float32(pc0 + k * vs * osf)
        host_cell = int((float(x) - pc0) / vs / osf)
        f32_cell = int((np.float32(x - np.float32(pc0)) * inv_vs) * inv_osf)
        if host_cell == k - 1 and f32_cell == k:
            break
    else:
        pytest.fail("no boundary centre separates the two chains")
    boxes = [torch.tensor([[float(x), 0.5, 0.0, 2.0, 4.0, 1.5, 0.3, 0.0, 0.0]], device=dev)]
    labels = [torch.tensor([0], device=dev)]
    head = head.to(dev)
    host = head.get_targets(boxes, labels)
    got = head.get_targets_device(boxes, labels)
    ref = oracle(boxes, labels, NCLS, tc, True)
    assert_matches_oracle(got, ref)
    fw = tc["grid_size"][0] // osf
    assert int(got.inds[0, 0, 0]) % fw == k and int(host[2][0][0, 0]) % fw == k - 1


@gpu
def test_multitask_loss_with_device_targets(dev):
    cfg = dataclasses.replace(CFG_TINY, density_mode="sdf", final_dim=(192, 224), num_classes=6)
    torch.manual_seed(0)
    bb, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(cfg.sdf_bias)
    batch = M.synthetic_batch(cfg, 2, seed=5, device=dev, num_points=40, num_boxes=12)
    host_fn = M.MultiTaskLoss(model, sdf_bias=cfg.sdf_bias)
    dev_fn = M.MultiTaskLoss(model, sdf_bias=cfg.sdf_bias, det_targets="device")
    with torch.no_grad():
        out = model(batch[0], batch[1], inrange_pts=batch[11])
        preds = out[0]
        fresh = lambda: [[{k: v.clone() for k, v in pd[0].items()}] for pd in preds]
        h = model.loss(host_fn.targets(batch), fresh())
        d = model.loss(dev_fn.targets(batch), fresh())
    assert float(h) > 0 and abs(float(d) - float(h)) <= 1e-6 * abs(float(h))
    loss = M.multitask_step(model, dev_fn, batch, amp_dtype=torch.bfloat16)
    assert torch.isfinite(loss) and torch.isfinite(dev_fn.last["detection"])
