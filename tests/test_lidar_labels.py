"""Lidar points rasterised into camera and BEV training labels on the device (labels.lidar_labels over the HIP kernels
of lidar_labels.hip).

Two references.  tests/golden/lidar_labels.npz holds maps made by the reference loader's own depth_transform and
get_bev_seg_map (make_lidar_labels_golden.py).  The oracle below restates the rules of include/vampire_hip.h in numpy,
with a sort in place of the atomics: candidates ordered by (cell, depth, index) -- or (cell, -height, index) -- and
the first of every cell taken.  A CPU test holds the oracle to every map of the fixture, exactly; that is what licenses
using it in the GPU sweeps.

Exactness: every output is an integer, a bit pattern copied from an input or a boolean, and the chain is stated
operation by operation, so every comparison is torch.equal (depth and height as int32 bit patterns)."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, synthetic                      # noqa: E402
from vampire_amd import labels as L                          # noqa: E402
from vampire_amd.build import build_library                  # noqa: E402
from vampire_amd.config import CFG_TINY                      # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "lidar_labels.npz")
CAM_CASES = ("ident", "flip", "rot", "edge")
BEV_CASES = ("bev", "edgebev")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ----------------------------------------------------------------------------------------------------- the oracle
def cam_candidates(pts, n_pts, m, k, a, final_dim, raw_dim):
    """One sample, one camera: (index, final u, final v, depth) of the points that reach the full-resolution map."""
    H, W = final_dim
    raw_h, raw_w = raw_dim
    x, y, z = (pts[:n_pts, i] for i in range(3))
    assert x.dtype == f32 and m.dtype == f32 and k.dtype == f32 and a.dtype == np.float64
    with np.errstate(all="ignore"):
        xc, yc, zc = (m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3))
        below = k[2, 0] * xc + k[2, 1] * yc + k[2, 2] * zc
        u = (k[0, 0] * xc + k[0, 1] * yc + k[0, 2] * zc) / below
        v = (k[1, 0] * xc + k[1, 1] * yc + k[1, 2] * zc) / below
        alive = (zc > 0) & (u > 1) & (u < f32(raw_w - 1)) & (v > 1) & (v < f32(raw_h - 1))
        u, v = u * f32(a[0]), v * f32(a[0])
        u, v = u - f32(a[1]), v - f32(a[2])
        if a[3] != 0:
            u = f32(W) - u
        u, v = u - f32(W / 2), v - f32(H / 2)
        wide_u, wide_v = u.astype(np.float64), v.astype(np.float64)
        u, v = (a[4] * wide_u + a[5] * wide_v).astype(f32), (-a[5] * wide_u + a[4] * wide_v).astype(f32)
        u, v = u + f32(W / 2), v + f32(H / 2)
        assert u.dtype == f32 and v.dtype == f32 and zc.dtype == f32
        alive &= (u >= 0) & (u < f32(W)) & (v >= 0) & (v < f32(H))
    idx = np.flatnonzero(alive)
    return idx, u[idx], v[idx], zc[idx]


def first_of_each_cell(cell, rank, idx):
    """The winners: per cell the candidate with the smallest rank, the lowest index among equals."""
    order = np.lexsort((idx, rank, cell))
    cell = cell[order]
    head = np.ones(len(cell), bool)
    head[1:] = cell[1:] != cell[:-1]
    return order[head]


def cam_oracle(pts, lab, counts, l2c, K, aug, final_dim, raw_dim, stride):
    B, N = l2c.shape[:2]
    h, w = final_dim[0] // stride, final_dim[1] // stride
    depth, seg = np.zeros((B, N, h * w), f32), np.zeros((B, N, h * w), np.int64)
    for b in range(B):
        for n in range(N):
            idx, u, v, d = cam_candidates(pts[b], int(counts[b]), l2c[b, n], K[b, n], aug[b, n], final_dim, raw_dim)
            iu, iv = u.astype(np.int64), v.astype(np.int64)
            on = (iu % stride == 0) & (iv % stride == 0)
            idx, d, cell = idx[on], d[on], (iv[on] // stride) * w + iu[on] // stride
            win = first_of_each_cell(cell, d, idx)
            depth[b, n, cell[win]] = d[win]
            seg[b, n, cell[win]] = lab[b, idx[win]].astype(np.int64) & 0xFF
    depth = depth.reshape(B, N, h, w)
    return depth, seg.reshape(B, N, h, w), depth > 0


def bev_candidates(pts, n_pts, grid):
    x_lo, x_hi, y_lo, y_hi, z_lo, z_hi, size = (float(g) for g in grid)
    nx, ny = int((x_hi - x_lo) / size), int((y_hi - y_lo) / size)
    p = pts[:n_pts]
    with np.errstate(all="ignore"):
        cx = (p[:, 0].astype(np.float64) - (x_lo - size / 2.0)) / size
        cy = (p[:, 1].astype(np.float64) - (y_lo - size / 2.0)) / size
        alive = (cx > 1) & (cx < nx - 1) & (cy > 1) & (cy < ny - 1) & (p[:, 2] > f32(z_lo)) & (p[:, 2] < f32(z_hi))
    idx = np.flatnonzero(alive)
    return idx, cy[idx].astype(np.int64) * nx + cx[idx].astype(np.int64), p[idx, 2], ny, nx


def bev_oracle(pts, lab, counts, grid):
    B = pts.shape[0]
    out = None
    for b in range(B):
        idx, cell, z, ny, nx = bev_candidates(pts[b], int(counts[b]), grid)
        if out is None:
            out = np.zeros((B, ny * nx), np.int64), np.zeros((B, ny * nx), f32), np.zeros((B, ny * nx), bool)
        win = first_of_each_cell(cell, -z.astype(np.float64), idx)
        out[0][b, cell[win]] = lab[b, idx[win]].astype(np.int64) & 0xFF
        out[1][b, cell[win]] = z[win]
        out[2][b, cell[win]] = True
    return tuple(o.reshape(B, 1, 1, ny, nx) for o in out)


def bev_dict(grid):
    g = [float(v) for v in grid]
    return dict(x_bound=(g[0], g[1]), y_bound=(g[2], g[3]), z_bound=(g[4], g[5]), size=g[6])


def golden_cam(name):
    g = golden()
    src = "edge" if name == "edge" else "cam"
    return dict(pts=g[f"{src}_points"], lab=g[f"{src}_labels"], counts=g[f"{src}_counts"], l2c=g[f"{name}_lidar2cam"],
                K=g[f"{name}_intrin"], aug=g[f"{name}_aug"], final_dim=tuple(int(v) for v in g["final_dim"]),
                raw_dim=tuple(int(v) for v in g[f"{name}_raw_dim"]))


# ----------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(**kw):
    d = _capi.VampLidarLabelDesc()
    d.B, d.N, d.M, d.point_cols, d.label_dtype = 2, 3, 0, 3, _capi.VAMP_U8
    d.H, d.W, d.stride, d.raw_w, d.raw_h, d.ny, d.nx = 16, 44, 2, 100, 40, 16, 16
    d.origin_x, d.origin_y, d.size, d.z_lo, d.z_hi = -3.4, -3.4, 0.4, -5.0, 3.0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_points_reject_bad_arguments_without_gpu(lib):
    assert C.sizeof(_capi.VampLidarLabelDesc) == 88
    fake = [C.c_void_p(0x1000 * (i + 1)) for i in range(13)]         # never dereferenced: every check comes first
    call = lambda d, a, nbytes=1 << 40: lib.vamp_lidar_labels(C.byref(d), *a, nbytes, None)
    zero = _capi.VampLidarLabelDesc()
    assert lib.vamp_lidar_labels_workspace_bytes(C.byref(zero)) == 0
    assert lib.vamp_lidar_labels_workspace_bytes(None) == 0
    assert call(zero, fake) == -1 and b"B must be in [1, 4096]" in lib.vamp_last_error()
    for field, value, message in (("stride", 3, b"stride must be positive and divide H and W"),
                                  ("stride", 0, b"stride must be positive"), ("N", 17, b"N must be in [1, 16]"),
                                  ("M", (1 << 24) + 1, b"M must be in [0, 2^24]"), ("point_cols", 5, b"point_cols"),
                                  ("label_dtype", _capi.VAMP_I32, b"label_dtype"), ("W", 8193, b"H, W must be"),
                                  ("nx", 0, b"ny, nx must be"), ("size", 0.0, b"size must be positive"),
                                  ("z_hi", -5.0, b"z_lo must be below z_hi")):
        bad = _desc(**{field: value})
        assert lib.vamp_lidar_labels_workspace_bytes(C.byref(bad)) == 0, field
        assert call(bad, fake) == -1 and message in lib.vamp_last_error(), (field, lib.vamp_last_error())
    d = _desc()
    need = lib.vamp_lidar_labels_workspace_bytes(C.byref(d))
    assert need == 2 * 3 * 8 * 22 * 8 + 2 * 16 * 16 * 8              # 8 bytes per cell, both 256-byte multiples here
    no_out = fake[:6] + [None] * 6 + fake[12:]
    assert call(d, no_out) == -1 and b"all NULL" in lib.vamp_last_error()
    partial = fake[:6] + [fake[6], None, fake[8]] + fake[9:]
    assert call(d, partial) == -1 and b"NULL together" in lib.vamp_last_error()
    no_aug = fake[:5] + [None] + fake[6:]
    assert call(d, no_aug) == -1 and b"lidar2cam, intrin or aug is NULL" in lib.vamp_last_error()
    assert call(_desc(M=5), [None] + fake[1:]) == -1 and b"points or labels is NULL" in lib.vamp_last_error()
    assert call(d, fake, need - 1) == -2 and b"workspace" in lib.vamp_last_error()
    assert call(d, fake[:12] + [None], need) == -2
    bev_only = fake[:3] + [None] * 6 + fake[9:]
    assert call(d, bev_only, need - 1) == -2                          # (the camera inputs are not asked for)
    with pytest.raises(_capi.VampireHipError, match="vamp_lidar_labels failed with code -1"):
        _capi.checked().vamp_lidar_labels(zero, *([None] * 13), 0, None)


def test_python_interface_refuses_cpu_tensors_and_wrong_arguments():
    pts, lab = torch.zeros(2, 5, 3), torch.zeros(2, 5, dtype=torch.uint8)
    bev = dict(x_bound=(-3.2, 3.2), y_bound=(-3.2, 3.2))
    with pytest.raises(_capi.VampireHipError):
        L.lidar_labels(pts, lab, bev=bev)
    with pytest.raises(_capi.VampireHipError):
        L.lidar_labels([pts[0], pts[1]], [lab[0], lab[1]], bev=bev)
    with pytest.raises(ValueError):
        L.lidar_labels([pts[0]], [lab[0], lab[1]], bev=bev)
    with pytest.raises(ValueError):
        L.lidar_labels(pts, [lab[0], lab[1]], bev=bev)


def test_ida_table_and_lidar2cam_on_a_hand_case():
    augs = [[(0.5, (50, 20), (3, 2, 47, 18), True, 90.0), (1.0, (44, 16), (0, 0, 44, 16), False, 0)]]
    t = L.ida_table(augs, "cpu")
    assert t.dtype == torch.float64 and tuple(t.shape) == (1, 2, 8)
    assert t[0, 0].tolist() == [0.5, 3.0, 2.0, 1.0, float(np.cos(90.0 / 180 * np.pi)), 1.0, 0.0, 0.0]
    assert t[0, 1].tolist() == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    angle = 5.4 / 180 * np.pi
    t = L.ida_table([[(0.5, None, (0, 0), 0, 5.4)]], "cpu")
    assert t[0, 0, 4].item() == np.cos(angle) and t[0, 0, 5].item() == np.sin(angle)
    with pytest.raises(ValueError):
        L.ida_table([], "cpu")
    # a camera one (1, 2, 3) from the ego origin, axes aligned; bda: a quarter turn about z
    s2e = torch.eye(4).repeat(1, 1, 2, 1, 1)
    s2e[0, 0, :, :3, 3] = torch.tensor([1.0, 2.0, 3.0])
    bda = synthetic.bda_matrix(1, rot_deg=90.0)
    m = L.lidar2cam_from_mats(dict(sensor2ego_mats=s2e, bda_mat=bda))
    assert m.dtype == torch.float32 and tuple(m.shape) == (1, 2, 4, 4)
    got = m[0, 1].double() @ torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=torch.float64)    # ego (1, 0, 0) after the turn
    assert torch.allclose(got, torch.tensor([0.0, -2.0, -3.0, 1.0], dtype=torch.float64), atol=1e-6)


@pytest.mark.parametrize("name", CAM_CASES)
def test_oracle_reproduces_the_reference_camera_maps(name):
    g, c = golden(), golden_cam(name)
    for stride in (1, 2):
        depth, seg, fg = cam_oracle(stride=stride, **c)
        want_d, want_s = g[f"{name}_depth"][..., ::stride, ::stride], g[f"{name}_seg"][..., ::stride, ::stride]
        assert np.array_equal(depth.view(np.int32), np.ascontiguousarray(want_d).view(np.int32)), (name, stride)
        assert np.array_equal(seg, want_s.astype(np.int64)) and np.array_equal(fg, want_d > 0), (name, stride)
        assert fg.sum() > 0


@pytest.mark.parametrize("name", BEV_CASES)
def test_oracle_reproduces_the_reference_bev_maps(name):
    g = golden()
    seg, height, mask = bev_oracle(g[f"{name}_points"], g[f"{name}_labels"], g[f"{name}_counts"], g[f"{name}_grid"])
    assert np.array_equal(seg[:, 0, 0], g[f"{name}_seg"].astype(np.int64))
    assert np.array_equal(height[:, 0, 0].view(np.int32), g[f"{name}_height"].view(np.int32))
    assert np.array_equal(mask[:, 0, 0], g[f"{name}_mask"]) and mask.sum() > 0


def _shared(cells, values):
    pairs = np.stack([cells.astype(np.float64), values.astype(np.float64)], 1)
    assert len(np.unique(pairs, axis=0)) == len(pairs), "two candidates of one cell share a depth / height"
    _, n = np.unique(cells, return_counts=True)
    return float((n >= 2).mean())


def test_fixture_conditions_hold():
    """No ties inside a cell, enough contested cells, no rotated coordinate near an integer, ragged counts."""
    g = golden()
    counts = g["cam_counts"]
    assert counts[1] == 0 and all(int(c) % 256 for c in counts[[0, 2]]) and counts[0] != counts[2]
    for name in CAM_CASES:
        c = golden_cam(name)
        H, W = c["final_dim"]
        cells, vals = [], []
        for b in range(c["l2c"].shape[0]):
            for n in range(c["l2c"].shape[1]):
                idx, u, v, d = cam_candidates(c["pts"][b], int(c["counts"][b]), c["l2c"][b, n], c["K"][b, n],
                                              c["aug"][b, n], c["final_dim"], c["raw_dim"])
                cells.append(((b * 16 + n) * H + v.astype(np.int64)) * W + u.astype(np.int64))
                vals.append(d)
                if name == "rot" and len(u):
                    assert c["aug"][b, n, 5] != 0
                    assert min(np.abs(u - np.round(u)).min(), np.abs(v - np.round(v)).min()) > 1e-3
        shared = _shared(np.concatenate(cells), np.concatenate(vals))
        assert name == "edge" or shared >= 0.25, (name, shared)
    for name in BEV_CASES:
        cells, vals = [], []
        for b in range(len(g[f"{name}_counts"])):
            idx, cell, z, ny, nx = bev_candidates(g[f"{name}_points"][b], int(g[f"{name}_counts"][b]), g[f"{name}_grid"])
            cells.append(b * ny * nx + cell)
            vals.append(z)
        shared = _shared(np.concatenate(cells), np.concatenate(vals))
        assert name == "edgebev" or shared >= 0.25, (name, shared)
    # the edges land where the arithmetic says
    lands = np.zeros(len(g["edge_lands"]), bool)
    lands[np.unique(g["edge_seg"][g["edge_seg"] > 0]) - 1] = True
    assert not (lands & ~g["edge_lands"]).any() and lands.sum() == 3


# ----------------------------------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def to_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run(dev, pts, lab, counts, l2c=None, K=None, aug=None, final_dim=None, raw_dim=None, stride=1, grid=None, **kw):
    return L.lidar_labels(to_dev(pts, dev), to_dev(lab, dev), counts=to_dev(counts, dev), lidar2cam=to_dev(l2c, dev),
                          intrins=to_dev(K, dev), aug=to_dev(aug, dev), final_dim=final_dim, raw_dim=raw_dim,
                          stride=stride if l2c is not None else 1, bev=None if grid is None else bev_dict(grid), **kw)


def bits(t):
    return t.contiguous().view(torch.int32).cpu()


def assert_cam(out, depth, seg, fg, what=""):
    assert out.cam_depth.dtype == torch.float32 and out.cam_seg.dtype == torch.int64 and out.cam_fg.dtype == torch.bool
    assert torch.equal(bits(out.cam_depth), torch.from_numpy(np.ascontiguousarray(depth).view(np.int32))), what
    assert torch.equal(out.cam_seg.cpu(), torch.from_numpy(np.ascontiguousarray(seg).astype(np.int64))), what
    assert torch.equal(out.cam_fg.cpu(), torch.from_numpy(np.ascontiguousarray(fg))), what


def assert_bev(out, seg, height, mask, what=""):
    assert out.bev_seg.dtype == torch.int64 and out.bev_height.dtype == torch.float32 and out.bev_mask.dtype == torch.bool
    assert torch.equal(out.bev_seg.cpu(), torch.from_numpy(np.ascontiguousarray(seg).astype(np.int64))), what
    assert torch.equal(bits(out.bev_height), torch.from_numpy(np.ascontiguousarray(height).view(np.int32))), what
    assert torch.equal(out.bev_mask.cpu(), torch.from_numpy(np.ascontiguousarray(mask))), what


def assert_same(a, b, what=""):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert (x is None) == (y is None), (what, f.name)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape, (what, f.name)
            x, y = (bits(t) if t.dtype == torch.float32 else t.cpu() for t in (x, y))
            assert torch.equal(x, y), (what, f.name)


@gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", CAM_CASES)
def test_fixture_camera_maps(dev, name, stride):
    """Every camera case of the fixture (the edges in exact arithmetic among them) with the fixture's BEV cloud's grid
    in the same call; then the camera-only call, which must equal the combined one."""
    g, c = golden(), golden_cam(name)
    out = run(dev, stride=stride, grid=g["bev_grid"], **c)
    want_d = g[f"{name}_depth"][..., ::stride, ::stride]
    assert_cam(out, want_d, g[f"{name}_seg"][..., ::stride, ::stride], want_d > 0, name)
    assert_bev(out, *bev_oracle(c["pts"], c["lab"], c["counts"], g["bev_grid"]), name)
    alone = run(dev, stride=stride, **c)
    assert alone.bev_seg is None and alone.bev_height is None and alone.bev_mask is None
    for f in ("cam_depth", "cam_seg", "cam_fg"):
        assert torch.equal(getattr(alone, f), getattr(out, f)), f


@gpu
@pytest.mark.parametrize("name", BEV_CASES)
def test_fixture_bev_maps(dev, name):
    g, c = golden(), golden_cam("flip")
    pts, lab, counts, grid = (g[f"{name}_{k}"] for k in ("points", "labels", "counts", "grid"))
    alone = run(dev, pts, lab, counts, grid=grid)
    assert alone.cam_depth is None and alone.cam_seg is None and alone.cam_fg is None
    assert tuple(alone.bev_seg.shape) == (len(counts), 1, 1) + g[f"{name}_seg"].shape[1:]
    assert_bev(alone, g[f"{name}_seg"][:, None, None], g[f"{name}_height"][:, None, None], g[f"{name}_mask"][:, None, None])
    # combined with cameras (the BEV cloud seen by the first samples' rig): the BEV part does not change
    B = len(counts)
    cam = dict(l2c=c["l2c"][:B], K=c["K"][:B], aug=c["aug"][:B], final_dim=c["final_dim"], raw_dim=c["raw_dim"])
    both = run(dev, pts, lab, counts, grid=grid, **cam)
    for f in ("bev_seg", "bev_height", "bev_mask"):
        assert torch.equal(getattr(alone, f), getattr(both, f)), f
    assert_cam(both, *cam_oracle(pts, lab, counts, stride=1, **cam))


# ---- random scenes ----------------------------------------------------------------------------------------------
FINAL, RAW = (32, 88), (900, 1600)
GRID = (-12.8, 12.8, -6.4, 6.4, -0.5, 3.0, 0.8)               # 16 rows (y) x 32 columns (x): not square


def scene(B, N, M, cols=3, lab_dtype=np.uint8, seed=0, counts=None, rotate=True):
    """A rig of N cameras per sample (bda: a turn and a scale), M points per sample in the bda frame, random
    train-mode augmentations with a rotation."""
    rng = np.random.default_rng(seed)
    cfg = dataclasses.replace(CFG_TINY, num_cams=N)
    s2e, K, _ = synthetic.camera_rig(cfg, B, jitter=1.0, seed=seed)
    l2c = L.lidar2cam_from_mats(dict(sensor2ego_mats=s2e, bda_mat=synthetic.bda_matrix(B, rot_deg=10.0, scale=1.05)))
    pts = np.concatenate([rng.uniform(-14, 14, (B, M, 2)), rng.uniform(-1.0, 3.5, (B, M, 1)),
                          rng.uniform(0, 255, (B, M, cols - 3))], 2).astype(f32)
    lab = rng.integers(0, 256, (B, M)).astype(np.uint8) if lab_dtype == np.uint8 else rng.integers(-3, 600, (B, M))
    augs = []
    for b in range(B):
        row = []
        for n in range(N):
            resize = float(rng.uniform(0.056, 0.07))
            new_w, new_h = int(RAW[1] * resize), int(RAW[0] * resize)
            cw, ch = int(rng.integers(0, new_w - FINAL[1] + 1)), int(rng.integers(0, new_h - FINAL[0] + 1))
            row.append((resize, (new_w, new_h), (cw, ch, cw + FINAL[1], ch + FINAL[0]), bool(rng.integers(0, 2)),
                        float(rng.uniform(-5.4, 5.4)) if rotate else 0))
        augs.append(row)
    if counts is None:
        counts = [M, 0, M - M // 3][:B] if B == 3 else [M] * B
    return dict(pts=pts, lab=lab, counts=np.asarray(counts, np.int32), l2c=l2c.numpy(), K=K.numpy(),
                aug=L.ida_table(augs, "cpu").numpy(), final_dim=FINAL, raw_dim=RAW)


@gpu
@pytest.mark.parametrize("M", [0, 1, 255, 256, 257, 3000])
@pytest.mark.parametrize("N", [1, 6, 16])
def test_random_sweep_against_the_oracle(dev, N, M):
    """Three samples, the middle one empty, rotated augmentations; per (N, M) every stride, and the label dtype and
    the point columns alternate so that each meets every N and every M's neighbour."""
    i = [1, 6, 16].index(N) + [0, 1, 255, 256, 257, 3000].index(M)
    sc = scene(3, N, M, cols=3 + i % 2, lab_dtype=np.uint8 if (i // 2) % 2 else np.int64, seed=100 + 7 * i)
    assert (sc["aug"][..., 5] != 0).all()
    want_bev = bev_oracle(sc["pts"], sc["lab"], sc["counts"], GRID)
    written = 0
    for stride in (1, 2, 4):
        out = run(dev, stride=stride, grid=GRID, **sc)
        want = cam_oracle(stride=stride, **sc)
        assert tuple(out.cam_depth.shape) == (3, N, FINAL[0] // stride, FINAL[1] // stride)
        assert tuple(out.bev_seg.shape) == (3, 1, 1, 16, 32)
        assert_cam(out, *want, (N, M, stride))
        assert_bev(out, *want_bev, (N, M, stride))
        assert not out.cam_fg[1].any() and not out.bev_mask[1].any()
        written += int(want[2].sum())
    if M >= 255:
        assert written > 0 and want_bev[2].sum() > 0


@gpu
def test_non_finite_huge_and_denormal_points_fall_out(dev):
    sc = scene(2, 6, 1500, seed=11, counts=[1500, 1200])
    good = run(dev, grid=GRID, **sc)
    nan, inf, big, tiny = f32(np.nan), f32(np.inf), f32(1e30), f32(1e-40)
    bad = np.array([[nan, tiny, tiny], [tiny, nan, 1.0], [1.0, 2.0, nan], [inf, tiny, tiny], [tiny, -inf, 1.0],
                    [2.0, 1.0, inf], [-inf, inf, -inf], [big, big, big], [0.0, tiny, big], [-big, big, -big],
                    [nan, nan, nan], [inf, inf, inf]], f32)
    assert tiny > 0 and tiny < np.finfo(f32).tiny
    # spread through both samples; the valid points keep their order (their indices move: no ties here to notice)
    where = np.linspace(0, 1100, len(bad)).astype(int)
    pts = np.stack([np.insert(sc["pts"][b], where, bad, axis=0) for b in range(2)])
    lab = np.stack([np.insert(sc["lab"][b], where, 7) for b in range(2)])
    mixed = dict(sc, pts=pts, lab=lab, counts=sc["counts"] + len(bad))
    out = run(dev, grid=GRID, **mixed)
    assert_same(out, good)
    assert_cam(out, *cam_oracle(stride=1, **mixed))
    # a point whose coordinates are all denormal is an ordinary point at the origin: the oracle says where it lands
    origin = dict(sc, pts=np.concatenate([sc["pts"], np.full((2, 1, 3), tiny)], 1),
                  lab=np.concatenate([sc["lab"], np.full((2, 1), 9, np.uint8)], 1), counts=np.array([1501, 1501], np.int32))
    origin["pts"][1, 1200:1500] = nan
    out = run(dev, grid=GRID, **origin)
    assert_cam(out, *cam_oracle(stride=1, **origin))
    seg, height, mask = bev_oracle(origin["pts"], origin["lab"], origin["counts"], GRID)
    assert_bev(out, seg, height, mask)
    assert mask[0, 0, 0, 8, 16]


@gpu
def test_equal_depths_and_heights_go_to_the_lowest_index(dev):
    """Two and three points of one cell with identical depth (height) and different labels, in several orders."""
    g = golden()
    l2c = K = np.eye(4, dtype=f32)[None, None]                 # u = x / z, v = y / z
    aug = np.array([[[1.0, 0, 0, 0, 1.0, 0.0, 0, 0]]])
    cam = dict(l2c=l2c, K=K, aug=aug, final_dim=(16, 44), raw_dim=(40, 100))
    grid = g["edgebev_grid"]
    # pixel (5, 7) at depth 2, three sub-pixel positions; a nearer and a farther point elsewhere and in the same pixel
    same = [(7.25, 5.5, 2.0), (7.5, 5.25, 2.0), (7.75, 5.75, 2.0)]
    far, other = (7.5, 5.5, 4.0), (20.5, 9.5, 2.0)
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0], [0, 1], [1, 0], [2, 0]):
        rows = [far] + [same[i] for i in order] + [other]
        pts = np.array([[u * z, v * z, z] for u, v, z in rows], f32)[None]
        lab = np.arange(10, 10 + len(rows), dtype=np.uint8)[None]
        out = run(dev, pts, lab, np.array([len(rows)], np.int32), **cam)
        assert out.cam_seg[0, 0, 5, 7].item() == 11 and out.cam_depth[0, 0, 5, 7].item() == 2.0, order
        assert out.cam_seg[0, 0, 9, 20].item() == 10 + len(rows) - 1 and int(out.cam_fg.sum()) == 2
        assert_cam(out, *cam_oracle(pts, lab, [len(rows)], stride=1, **cam))
    # BEV cell (8, 8) of the dyadic grid at height 1.5, a lower point first
    same = [(0.0, 0.0, 1.5), (0.125, 0.0625, 1.5), (0.0625, 0.125, 1.5)]
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0], [0, 1], [1, 0], [2, 0]):
        rows = [(0.1, 0.1, -2.0)] + [same[i] for i in order] + [(2.0, 1.0, 1.5)]
        pts = np.array(rows, f32)[None]
        lab = np.arange(20, 20 + len(rows), dtype=np.int64)[None]
        out = run(dev, pts, lab, np.array([len(rows)], np.int32), grid=grid)
        assert out.bev_seg[0, 0, 0, 8, 8].item() == 21 and out.bev_height[0, 0, 0, 8, 8].item() == 1.5, order
        assert int(out.bev_mask.sum()) == 2
        assert_bev(out, *bev_oracle(pts, lab, [len(rows)], grid))


@gpu
def test_a_permuted_cloud_gives_identical_maps(dev):
    sc = scene(2, 6, 3000, seed=5, counts=[3000, 3000])
    for b in range(2):                                         # tie-free: no two candidates of a cell share a value
        for n in range(6):
            _, u, v, d = cam_candidates(sc["pts"][b], 3000, sc["l2c"][b, n], sc["K"][b, n], sc["aug"][b, n], FINAL, RAW)
            _shared(v.astype(np.int64) * FINAL[1] + u.astype(np.int64), d)
        _, cell, z, _, _ = bev_candidates(sc["pts"][b], 3000, GRID)
        _shared(cell, z)
    want = cam_oracle(stride=1, **sc)
    cells = want[2].sum()
    first = run(dev, grid=GRID, **sc)
    assert_cam(first, *want)
    rng = np.random.default_rng(1)
    for _ in range(2):
        perm = np.stack([rng.permutation(3000) for _ in range(2)])
        moved = dict(sc, pts=np.take_along_axis(sc["pts"], perm[..., None], 1), lab=np.take_along_axis(sc["lab"], perm, 1))
        assert_same(run(dev, grid=GRID, **moved), first)
    assert cells > 500


@gpu
def test_dirty_workspace_and_out_reuse_are_bitwise_repeatable(dev):
    from vampire_amd import _tensors
    sc = scene(3, 6, 3000, seed=9)
    first = run(dev, stride=2, grid=GRID, **sc)
    want = cam_oracle(stride=2, **sc)
    assert_cam(first, *want)
    keys = [k for k in _tensors._scratch if isinstance(k, tuple) and k[0] == "lidar_labels"]
    assert keys
    keep = dataclasses.replace(first, **{f.name: getattr(first, f.name).clone() for f in dataclasses.fields(first)})
    out = L.LidarLabels(**{f.name: torch.empty_like(getattr(first, f.name)) for f in dataclasses.fields(first)})
    for _ in range(3):
        for k in keys:
            _tensors._scratch[k].fill_(0xA5)
        for f in dataclasses.fields(out):
            getattr(out, f.name).view(torch.uint8).fill_(0xA5)
        ptrs = [getattr(out, f.name).data_ptr() for f in dataclasses.fields(out)]
        got = run(dev, stride=2, grid=GRID, out=out, **sc)
        assert got is out and ptrs == [getattr(out, f.name).data_ptr() for f in dataclasses.fields(out)]
        assert_same(out, keep)
    with pytest.raises(ValueError):
        run(dev, stride=1, grid=GRID, out=out, **sc)            # buffers of another shape


@gpu
def test_layouts_give_the_same_values_or_raise(dev):
    sc = scene(2, 6, 2000, cols=4, seed=13, counts=[2000, 1500])
    t = {k: to_dev(sc[k], dev) for k in ("pts", "lab", "counts", "l2c", "K", "aug")}
    kw = dict(final_dim=FINAL, raw_dim=RAW, stride=1, bev=bev_dict(GRID))
    call = lambda **ch: L.lidar_labels(ch.get("pts", t["pts"]), ch.get("lab", t["lab"]), counts=t["counts"],
                                       lidar2cam=ch.get("l2c", t["l2c"]), intrins=t["K"], aug=ch.get("aug", t["aug"]), **kw)
    plain = call()
    assert_cam(plain, *cam_oracle(stride=1, **sc))
    wide = torch.zeros(2, 2000, 8, device=dev)
    wide[..., :4] = t["pts"]
    off = torch.zeros(2 * 2000 * 4 + 1, device=dev)
    off[1:] = t["pts"].reshape(-1)
    lab_off = torch.zeros(2 * 2000 + 3, dtype=torch.uint8, device=dev)
    lab_off[3:] = t["lab"].reshape(-1)
    aug_t = t["aug"].transpose(1, 2).contiguous().transpose(1, 2)
    views = dict(strided=dict(pts=wide[..., :4]), misaligned=dict(pts=off[1:].view(2, 2000, 4)),
                 labels_misaligned=dict(lab=lab_off[3:].view(2, 2000)),
                 transposed_l2c=dict(l2c=t["l2c"].transpose(2, 3).contiguous().transpose(2, 3)), strided_aug=dict(aug=aug_t))
    assert not views["strided"]["pts"].is_contiguous() and views["misaligned"]["pts"].data_ptr() % 16 == 4
    assert not views["transposed_l2c"]["l2c"].is_contiguous() and not aug_t.is_contiguous()
    for name, ch in views.items():
        try:
            got = call(**ch)
        except (ValueError, TypeError, _capi.VampireHipError):
            continue
        assert_same(got, plain, name)
    # an expanded tensor: both samples see sample 0's cloud
    one = dict(sc, pts=np.repeat(sc["pts"][:1], 2, 0), lab=np.repeat(sc["lab"][:1], 2, 0))
    try:
        got = call(pts=t["pts"][:1].expand(2, 2000, 4), lab=t["lab"][:1].expand(2, 2000))
    except (ValueError, TypeError, _capi.VampireHipError):
        return
    assert_cam(got, *cam_oracle(stride=1, **one))
    assert_bev(got, *bev_oracle(one["pts"], one["lab"], one["counts"], GRID))


@gpu
def test_no_sync_and_graph_replay(dev):
    """The list call and the packed call under the sync debug mode; then this operator alone in a graph, its points,
    labels, counts and augmentation table overwritten in place before every replay."""
    sc = scene(3, 6, 3000, seed=21)
    pts, lab, counts, l2c, K, aug = (to_dev(sc[k], dev) for k in ("pts", "lab", "counts", "l2c", "K", "aug"))
    kw = dict(lidar2cam=l2c, intrins=K, aug=aug, final_dim=FINAL, raw_dim=RAW, stride=2, bev=bev_dict(GRID))
    lists = [pts[b, :int(sc["counts"][b])].clone() for b in range(3)], [lab[b, :int(sc["counts"][b])].clone() for b in range(3)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = L.lidar_labels(*lists, **kw)
        out = L.lidar_labels(pts, lab, counts=counts, **kw)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            L.lidar_labels(pts, lab, counts=counts, out=out, **kw)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            L.lidar_labels(pts, lab, counts=counts, out=out, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert_same(eager, out)
    assert_cam(out, *cam_oracle(stride=2, **sc))
    for seed in (5, 6, 7):
        fresh = scene(3, 6, 3000, seed=seed, counts=[3000 - 100 * seed, 17 * seed, 0])
        pts.copy_(to_dev(fresh["pts"], dev))
        lab.copy_(to_dev(fresh["lab"], dev))
        counts.copy_(to_dev(fresh["counts"], dev))
        aug.copy_(to_dev(fresh["aug"], dev))
        g.replay()
        ref = L.lidar_labels(pts, lab, counts=counts, **kw)
        torch.cuda.synchronize()
        assert_same(ref, out, seed)
        fresh.update(l2c=sc["l2c"], K=sc["K"])
        assert_cam(out, *cam_oracle(stride=2, **fresh), seed)
        assert int(out.cam_fg.sum()) > 0 and int(out.bev_mask.sum()) > 0


@gpu
def test_fill_train_labels_feeds_the_losses(dev):
    from vampire_amd import multitask as M
    from vampire_amd import ops
    cfg = CFG_TINY
    batch = M.synthetic_batch(cfg, 2, seed=3, device=dev, num_points=2000)
    H, W = cfg.final_dim
    resize = max(H / 900, W / 1600)                            # the rig's own "val" augmentation
    new_w, new_h = int(1600 * resize), int(900 * resize)
    aug = (resize, (new_w, new_h), (0, new_h - H, W, new_h), False, 0)
    augs = [[aug] * cfg.num_cams] * 2
    full = L.fill_train_labels(batch, cfg, augs)
    assert len(full) == len(batch)
    for i in range(len(batch)):
        if i in (6, 7, 8, 9, 10):
            assert full[i].shape == batch[i].shape and full[i].dtype == batch[i].dtype and full[i].device == batch[i].device, i
        else:
            assert full[i] is batch[i], i
    assert int((full[6] > 0).sum()) > 100 and int(full[10].sum()) > 100
    # the labels are those of the batch's own geometry
    mats = batch[1]
    sc = dict(pts=np.stack([p.cpu().numpy() for p in batch[11]]), lab=np.stack([l.cpu().numpy() for l in batch[12]]),
              counts=np.array([2000, 2000], np.int32), l2c=L.lidar2cam_from_mats(mats).cpu().numpy(),
              K=mats["intrin_mats"][:, 0].cpu().numpy(), aug=L.ida_table(augs, "cpu").numpy(), final_dim=(H, W),
              raw_dim=(900, 1600))
    depth, seg, fg = cam_oracle(stride=1, **sc)
    assert torch.equal(bits(full[6][:, 0]), torch.from_numpy(depth.view(np.int32)))
    assert torch.equal(full[7][:, 0].cpu(), torch.from_numpy(seg))
    grid = (*cfg.x_bound_det[:2], *cfg.y_bound_det[:2], -5.0, 3.0, cfg.x_bound_det[2])
    b_seg, b_height, b_mask = bev_oracle(sc["pts"], sc["lab"], sc["counts"], grid)
    assert torch.equal(full[8].cpu(), torch.from_numpy(b_seg)) and torch.equal(full[10].cpu(), torch.from_numpy(b_mask))
    assert torch.equal(bits(full[9]), torch.from_numpy(b_height.view(np.int32)))
    # get_downsampled_gt's pick of the stride-1 labels is the stride-4 call
    quarter = L.fill_train_labels(batch, cfg, augs, stride=4)
    loss_fn = M.MultiTaskLoss(None, downsample_factor=16, upsample_factor=4)
    _, depth_l, seg_l, fg_l = loss_fn.downsampled_gt(batch[0][:, 0], full[6][:, 0], full[7][:, 0])
    assert torch.equal(bits(depth_l), bits(quarter[6][:, 0])) and torch.equal(seg_l, quarter[7][:, 0])
    assert torch.equal(fg_l, quarter[6][:, 0] > 0) and int(fg_l.sum()) > 20
    assert tuple(depth_l.shape) == (2, cfg.num_cams, H // 4, W // 4)
    # the segmentation loss takes them, on the device and as the host expression, as in test_seg_loss.py: the HIP
    # value may stand off the float64 value by at most twice what torch's own fp32 evaluation does (or 1e-6)
    torch.manual_seed(0)
    Kc = cfg.num_classes
    for logits, lab, mask in ((torch.randn(*seg_l.shape, Kc, device=dev), seg_l, fg_l),
                              (torch.randn(*full[8].shape, Kc, device=dev), full[8], full[10])):
        assert int(lab[mask].max()) < Kc
        hip = float(ops.seg_loss(logits, lab, mask))
        host = float(M._ce_lovasz(logits[mask], lab[mask]))
        exact = float(M._ce_lovasz(logits.double()[mask], lab[mask]))
        e_hip, e_host = abs(hip - exact) / abs(exact), abs(host - exact) / abs(exact)
        print(f"  seg loss: hip {hip:.7f} host {host:.7f} float64 {exact:.7f}  ({e_hip:.2e} against {e_host:.2e})")
        assert e_hip <= max(2 * e_host, 1e-6)
