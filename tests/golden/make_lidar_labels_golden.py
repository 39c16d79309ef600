#!/usr/bin/env python3
"""Golden maps for the lidar-point label rasteriser (tests/test_lidar_labels.py), made by the reference loader's own
`depth_transform` and `get_bev_seg_map` IN THIS CONTAINER.  The reference module cannot be imported (nuscenes-devkit,
mmcv and mmdet3d are absent), so /root/reference/src/datasets/nusc_det_seg_dataset.py is parsed with `ast` at run time
and only the definitions of those two functions are executed, with `np` and `torch`; this script holds none of their
text.  Stage 1 -- lidar2cam, intrinsics and the raw-image margins -- lives in classes of the absent devkit: it is
computed here, in numpy fp32, one rounding per operation, in the order include/vampire_hip.h states, and the surviving
(u, v, depth) rows go to the reference's depth_transform.  Stride-s labels are map[::s, ::s] of the maps stored here.
Run once here; the .npz travels, the reference does not.

The script asserts the conditions the test relies on: no two candidates of a cell share a depth / height (the
reference's order is undefined there), at least 25 % of the written cells of every non-edge case had two candidates
or more, and in the rotated case no final coordinate lies within 1e-3 of an integer (numpy's float64 matmul may or
may not fuse the multiply-add; that cannot move such a point to another pixel)."""
import ast
import os

import numpy as np
import torch

REF = "/root/reference/src/datasets/nusc_det_seg_dataset.py"
WANT = ("depth_transform", "get_bev_seg_map")
tree = ast.parse(open(REF).read())
defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
assert sorted(n.name for n in defs) == sorted(WANT)
ref = {"np": np, "torch": torch}
exec(compile(ast.Module(body=defs, type_ignores=[]), REF, "exec"), ref)

f32 = np.float32
H, W = 16, 44
rng = np.random.default_rng(20)


# ------------------------------------------------------------------------------------------------ stage 1, ours
def rig(yaws_deg, height=1.5):
    """lidar2cam [N, 4, 4] fp32: cameras at (0, 0, height) looking along the yaws, x right, y down, z forward."""
    out = []
    for yaw in yaws_deg:
        a = np.deg2rad(yaw)
        rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        s2e = np.eye(4)
        s2e[:3, :3] = rz @ np.array([[0, 0, 1.0], [-1.0, 0, 0], [0, -1.0, 0]])
        s2e[:3, 3] = (0.3 * np.cos(a), 0.3 * np.sin(a), height)
        out.append(np.linalg.inv(s2e))
    return np.stack(out).astype(f32)


def intrinsics(n, focal, cu, cv):
    k = np.zeros((n, 4, 4), f32)
    k[:, 0, 0] = k[:, 1, 1] = focal
    k[:, 0, 2], k[:, 1, 2] = cu, cv
    k[:, 2, 2] = k[:, 3, 3] = 1
    return k


def stage1(pts, m, k, raw_w, raw_h):
    x, y, z = (pts[:, i].astype(f32) for i in range(3))
    row = lambda r: ((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3]
    xc, yc, zc = row(0), row(1), row(2)
    with np.errstate(all="ignore"):
        den = (k[2, 0] * xc + k[2, 1] * yc) + k[2, 2] * zc
        u = ((k[0, 0] * xc + k[0, 1] * yc) + k[0, 2] * zc) / den
        v = ((k[1, 0] * xc + k[1, 1] * yc) + k[1, 2] * zc) / den
    assert u.dtype == f32 and zc.dtype == f32
    keep = (zc > 0) & (u > 1) & (u < f32(raw_w - 1)) & (v > 1) & (v < f32(raw_h - 1))
    return u, v, zc, keep


def final_uv(u, v, aug):
    """Where the kept points end up (for the conditions below only; the maps come from the reference)."""
    resize, _, crop, flip, rotate = aug
    u, v = u * f32(resize) - f32(crop[0]), v * f32(resize) - f32(crop[1])
    if flip:
        u = f32(W) - u
    u, v = u - f32(W / 2), v - f32(H / 2)
    h = rotate / 180 * np.pi
    ud, vd = u.astype(np.float64), v.astype(np.float64)
    u, v = (np.cos(h) * ud + np.sin(h) * vd).astype(f32), (-np.sin(h) * ud + np.cos(h) * vd).astype(f32)
    return u + f32(W / 2), v + f32(H / 2)


def check_cells(cells, values, what, min_shared):
    """cells: the candidates' cell ids, values: their depth / height."""
    pairs = np.stack([cells.astype(np.float64), values.astype(np.float64)], 1)
    assert len(np.unique(pairs, axis=0)) == len(pairs), f"{what}: two candidates of a cell share a value"
    _, n = np.unique(cells, return_counts=True)
    shared = float((n >= 2).mean()) if len(n) else 0.0
    assert shared >= min_shared, f"{what}: only {shared:.0%} of the written cells had >= 2 candidates"
    return shared


def camera_case(name, pts, labels, counts, l2c, k, raw_hw, augs, out, min_shared=0.25):
    B, N = l2c.shape[:2]
    raw_h, raw_w = raw_hw
    depth, seg = np.zeros((B, N, H, W), f32), np.zeros((B, N, H, W), np.uint8)
    cells, vals = [], []
    for b in range(B):
        for n in range(N):
            u, v, d, keep = stage1(pts[b, :counts[b]], l2c[b, n], k[b, n], raw_w, raw_h)
            rows = np.stack([u[keep], v[keep], d[keep]], 1).astype(f32)
            resize, _, crop, flip, rotate = augs[b][n]
            dm, lm = ref["depth_transform"](rows.copy(), labels[b, :counts[b]][keep].copy(), resize, (H, W), crop, flip,
                                            rotate)
            depth[b, n], seg[b, n] = dm.numpy(), lm.numpy()
            fu, fv = final_uv(u[keep], v[keep], augs[b][n])
            ok = (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
            cells.append(((b * N + n) * H + fv[ok].astype(np.int64)) * W + fu[ok].astype(np.int64))
            vals.append(d[keep][ok])
            if rotate and ok.any():
                for c in (fu[ok], fv[ok]):
                    assert np.abs(c - np.round(c)).min() > 1e-3
    cells, vals = np.concatenate(cells), np.concatenate(vals)
    shared = check_cells(cells, vals, name, min_shared)
    assert len(np.unique(cells)) == int((depth > 0).sum()), name     # our candidates' cells are the reference's
    table = np.zeros((B, N, 8))
    for b in range(B):
        for n in range(N):
            resize, _, crop, flip, rotate = augs[b][n]
            table[b, n, :6] = (resize, crop[0], crop[1], float(flip), np.cos(rotate / 180 * np.pi),
                               np.sin(rotate / 180 * np.pi))
    out.update({f"{name}_lidar2cam": l2c, f"{name}_intrin": k, f"{name}_aug": table,
                f"{name}_raw_dim": np.array(raw_hw, np.int32), f"{name}_depth": depth, f"{name}_seg": seg})
    print(f"{name}: {int((depth > 0).sum())} written cells, {shared:.0%} of them with >= 2 candidates")


out = {"final_dim": np.array([H, W], np.int32)}

# ------------------------------------------------------------------------------------------------ camera cases
B, N = 3, 3
raw = (40, 100)                                               # raw_h, raw_w
l2c = np.stack([rig((0 + j, 120 - j, -120 + 2 * j)) for j in (0.0, 7.0, -11.0)])
k_raw = np.stack([intrinsics(N, 60.0 + b, 50.3, 19.6 + 0.5 * b) for b in range(B)])
k_fin = np.stack([intrinsics(N, 26.0 + b, 22.1, 7.9 + 0.25 * b) for b in range(B)])
crop = lambda x, y: (x, y, x + W, y + H)
augs = {
    "ident": [[(1.0, (W, H), crop(0, 0), False, 0)] * N] * B,
    "flip": [[(0.5, (50, 20), crop(3 + n, 2 + (b + n) % 2), True, 0) for n in range(N)] for b in range(B)],
    "rot": [[(0.5 + 0.01 * n, (50, 20), crop(3 + n, 2), False, 5.4 - 2.0 * b * n) for n in range(N)] for b in range(B)],
}
want = [4000, 0, 2700]


def cloud(n):
    return np.concatenate([rng.uniform(-12, 12, (n, 2)), rng.uniform(0.4, 2.6, (n, 1))], 1).astype(f32)


clouds = []
for b in range(B):
    p = cloud(want[b])
    near = np.zeros(len(p), bool)                             # the rotated case's near-integer coordinates go
    for n in range(N):
        u, v, d, keep = stage1(p, l2c[b, n], k_raw[b, n], raw[1], raw[0])
        fu, fv = final_uv(u, v, augs["rot"][b][n])
        with np.errstate(invalid="ignore"):
            near |= keep & ((np.abs(fu - np.round(fu)) < 2e-3) | (np.abs(fv - np.round(fv)) < 2e-3))
    clouds.append(p[~near])
counts = np.array([len(p) for p in clouds], np.int32)
assert counts[1] == 0 and all(c % 256 for c in counts[[0, 2]]) and counts[0] != counts[2]
M = int(counts.max())
pts = np.zeros((B, M, 3), f32)
for b in range(B):
    pts[b, :counts[b]] = clouds[b]
labels = rng.integers(1, 18, (B, M)).astype(np.uint8)
out.update(cam_points=pts, cam_labels=labels, cam_counts=counts)
camera_case("ident", pts, labels, counts, l2c, k_fin, (H, W), augs["ident"], out)
camera_case("flip", pts, labels, counts, l2c, k_raw, raw, augs["flip"], out)
camera_case("rot", pts, labels, counts, l2c, k_raw, raw, augs["rot"], out)


# ------------------------------------------------------------------------------------------------ BEV case
def bev_case(name, pts, labels, counts, xb, yb, zb, size, out, min_shared=0.25):
    B = len(counts)
    nx, ny = int((xb[1] - xb[0]) / size), int((yb[1] - yb[0]) / size)
    seg, height, mask = np.zeros((B, ny, nx), np.uint8), np.zeros((B, ny, nx), f32), np.zeros((B, ny, nx), bool)
    cells, vals = [], []
    for b in range(B):
        p, l = torch.from_numpy(pts[b, :counts[b]].copy()), torch.from_numpy(labels[b, :counts[b]].copy())
        s, h, m = ref["get_bev_seg_map"](p, l, x_bound=xb, y_bound=yb, z_bound=zb, size=size)
        seg[b], height[b], mask[b] = s.numpy(), h.numpy(), m.numpy()
        q = pts[b, :counts[b]]
        cx = (q[:, 0].astype(np.float64) - (xb[0] - size / 2.0)) / size
        cy = (q[:, 1].astype(np.float64) - (yb[0] - size / 2.0)) / size
        ok = (cx > 1) & (cx < nx - 1) & (cy > 1) & (cy < ny - 1) & (q[:, 2] > f32(zb[0])) & (q[:, 2] < f32(zb[1]))
        cells.append((b * ny + cy[ok].astype(np.int64)) * nx + cx[ok].astype(np.int64))
        vals.append(q[ok, 2])
    cells, vals = np.concatenate(cells), np.concatenate(vals)
    shared = check_cells(cells, vals, name, min_shared)
    assert len(np.unique(cells)) == int(mask.sum()), name
    out.update({f"{name}_points": pts, f"{name}_labels": labels, f"{name}_counts": counts,
                f"{name}_grid": np.array([xb[0], xb[1], yb[0], yb[1], zb[0], zb[1], size], np.float64),
                f"{name}_seg": seg, f"{name}_height": height, f"{name}_mask": mask})
    print(f"{name}: {int(mask.sum())} written cells, {shared:.0%} of them with >= 2 candidates")


bc = np.array([1500, 700], np.int32)
bp = np.zeros((2, 1500, 3), f32)
for b in range(2):
    bp[b, :bc[b]] = np.concatenate([rng.uniform(-4, 4, (bc[b], 2)), rng.uniform(-6, 4, (bc[b], 1))], 1)
bl = rng.integers(1, 18, (2, 1500)).astype(np.int64)
bev_case("bev", bp, bl, bc, (-3.2, 3.2), (-3.2, 3.2), (-5., 3.), 0.4, out)

# ------------------------------------------------------------------------------------------------ edges, exact
# lidar2cam = identity, focal 1, centre 0: u = x / z, v = y / z; z a power of two, so every coordinate is exact.
# crop (4, 2): final u = u - 4, final v = v - 2.  Every row: (raw u, raw v, depth), and whether it lands.
edge_rows = [
    (1.0, 8.0, 1.0, False), (99.0, 8.0, 2.0, False),          # raw u exactly 1 and raw_w - 1: out
    (8.0, 1.0, 4.0, False), (8.0, 39.0, 8.0, False),          # raw v exactly 1 and raw_h - 1: out
    (4.0, 8.0, 1.0, True),                                    # final u exactly 0.0: in
    (48.0, 8.0, 2.0, False),                                  # final u exactly W: out
    (3.5, 8.0, 4.0, False),                                   # final u -0.5: out, although it truncates to 0
    (8.0, 2.0, 1.0, True), (8.0, 18.0, 2.0, False), (8.0, 1.5, 4.0, False),      # the same along v
    (47.75, 17.75, 8.0, True),                                # the last pixel
    (4.0, 8.5, 0.5, True), (4.0, 8.25, 0.25, True),           # three candidates of pixel (6, 0): the nearest wins
    (10.0, 10.0, -1.0, False), (10.0, 10.0, 0.0, False),      # behind the camera, and in its plane
]
ep = np.array([[u * z, v * z, z] for u, v, z, _ in edge_rows], f32)[None]
el = np.arange(1, len(edge_rows) + 1, dtype=np.uint8)[None]
ec = np.array([len(edge_rows)], np.int32)
e_l2c, e_k = np.eye(4, dtype=f32)[None, None], np.eye(4, dtype=f32)[None, None]
e_aug = [[(1.0, (100, 40), crop(4, 2), False, 0)]]
u, v, d, keep = stage1(ep[0], e_l2c[0, 0], e_k[0, 0], 100, 40)
assert np.array_equal(u[2:13], np.array([r[0] for r in edge_rows[2:13]], f32))        # exact, as designed
out.update(edge_points=ep, edge_labels=el, edge_counts=ec, edge_lands=np.array([r[3] for r in edge_rows]))
camera_case("edge", ep, el, ec, e_l2c, e_k, raw, e_aug, out, min_shared=0.0)
lands = np.zeros(len(edge_rows), bool)
lands[np.unique(out["edge_seg"][out["edge_seg"] > 0]) - 1] = True
# (rows 4 and 11 lose pixel (6, 0) to row 12: what the reference's map shows is the winner)
assert np.array_equal(lands | np.isin(np.arange(len(edge_rows)), (4, 11)), out["edge_lands"])
assert out["edge_seg"][0, 0, 6, 0] == 13 and out["edge_depth"][0, 0, 6, 0] == 0.25

# BEV edges on a dyadic grid: 16 x 16 cells of 0.5 m, origin -4.25: cx = (x + 4.25) / 0.5
bev_rows = [
    (-3.75, 0.0, 0.0, False), (3.25, 0.0, 0.5, False),        # cx exactly 1 and nx - 1: out
    (0.0, -3.75, 1.0, False), (0.0, 3.25, 1.5, False),        # cy likewise
    (-3.5, 0.0, 0.25, True), (3.0, 0.0, 0.75, True),          # cx 1.5 and 14.5: in
    (0.0, 0.0, -5.0, False), (0.0, 0.0, 3.0, False),          # z exactly at both bounds: out
    (0.0, 0.0, -4.75, True), (0.1, 0.1, 2.75, True), (0.2, 0.2, -1.0, True),     # one cell, the highest wins
]
gp = np.array([r[:3] for r in bev_rows], f32)[None]
gl = np.arange(1, len(bev_rows) + 1, dtype=np.int64)[None]
bev_case("edgebev", gp, gl, np.array([len(bev_rows)], np.int32), (-4., 4.), (-4., 4.), (-5., 3.), 0.5, out,
         min_shared=0.0)
got = np.zeros(len(bev_rows), bool)
got[np.unique(out["edgebev_seg"][out["edgebev_mask"]]) - 1] = True
assert np.array_equal(got | np.isin(np.arange(len(bev_rows)), (8, 10)), np.array([r[3] for r in bev_rows]))
assert out["edgebev_seg"][0, 8, 8] == 10 and out["edgebev_height"][0, 8, 8] == 2.75

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lidar_labels.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
