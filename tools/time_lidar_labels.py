"""Time the lidar-point label rasteriser (labels.lidar_labels / vamp_lidar_labels) against two formulations of the
same maps.

    python tools/time_lidar_labels.py [--iters 500] [--json profiles/lidar_labels.json]

Configurations: six 256 x 704 camera maps at stride 1 and 4 over a 256 x 256 and a 200 x 200 BEV grid of 0.4 m,
34 720 (one nuScenes sweep) and 300 000 points per sample, B = 1 and 8; the rig and the val-mode augmentation of
vampire_amd.synthetic, points uniform over the grid.
  hip_us     the packed call with out= buffers, device events around `iters` back-to-back calls
  graph_us   the same captured in a graph, ten calls per graph, replayed
  torch_us   a torch formulation on the same GPU: the same projection as tensor ops (fp32, float64 where the kernel
             uses it), int64 keys scatter_reduce_'d with 'amin' / 'amax' into the maps, then a gather of the labels
  numpy_us   the tool's own sort-and-assign restatement on the host, one sample (what a data loader's worker does)
No ratio is fixed in advance; the rows are what was measured.  scatter_bytes is an ESTIMATE: 64 bytes of memory
traffic for every atomic the scatter issues (a lone 8-byte atomic dirties one 64-byte line); the rate of such atomics
is not documented anywhere, so scatter_gbs puts the estimate over the whole call's time only as a yardstick.
torch_equal reports whether the torch formulation's maps equal the kernels' (no ties in these clouds).  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import labels as L, synthetic  # noqa: E402
from vampire_amd.config import CFG_A  # noqa: E402

RAW = (900, 1600)
FINAL = CFG_A.final_dim


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def timed_graph(fn, iters):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10):
            fn()
    return timed(g.replay, max(iters // 10, 5), warmup=3) / 10


def val_aug():
    H, W = FINAL
    resize = max(H / RAW[0], W / RAW[1])
    new_w, new_h = int(RAW[1] * resize), int(RAW[0] * resize)
    cw = int(max(0, new_w - W) / 2)
    return resize, (new_w, new_h), (cw, new_h - H, cw + W, new_h), False, 0


def make_inputs(B, M, side, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    s2e, K, _ = synthetic.camera_rig(CFG_A, B, jitter=1.0, seed=seed)
    half = side * 0.4 / 2
    lo, hi = torch.tensor([-half, -half, -3.0]), torch.tensor([half, half, 3.0])
    pts = (torch.rand(B, M, 3, generator=g) * (hi - lo) + lo).to(dev)
    lab = torch.randint(0, 17, (B, M), generator=g, dtype=torch.int64).to(dev)
    l2c = L.lidar2cam_from_mats(dict(sensor2ego_mats=s2e, bda_mat=synthetic.bda_matrix(B))).to(dev)
    aug = L.ida_table([[val_aug()] * CFG_A.num_cams] * B, dev)
    bev = dict(x_bound=(-half, half), y_bound=(-half, half), z_bound=(-5., 3.), size=0.4)
    counts = torch.full((B,), M, dtype=torch.int32, device=dev)
    return pts, lab, counts, l2c, K.to(dev), aug, bev


def project_torch(pts, l2c, K, aug, stride):
    """The kernel's chain as tensor ops: (valid [B, N, M], cell [B, N, M], depth [B, N, M])."""
    H, W = FINAL
    x, y, z = (pts[:, None, :, i] for i in range(3))
    m = l2c[:, :, :, :, None]
    xc, yc, zc = (((m[:, :, r, 0] * x + m[:, :, r, 1] * y) + m[:, :, r, 2] * z) + m[:, :, r, 3] for r in range(3))
    k = K[:, :, :, :, None]
    den = (k[:, :, 2, 0] * xc + k[:, :, 2, 1] * yc) + k[:, :, 2, 2] * zc
    u = ((k[:, :, 0, 0] * xc + k[:, :, 0, 1] * yc) + k[:, :, 0, 2] * zc) / den
    v = ((k[:, :, 1, 0] * xc + k[:, :, 1, 1] * yc) + k[:, :, 1, 2] * zc) / den
    ok = (zc > 0) & (u > 1) & (u < RAW[1] - 1) & (v > 1) & (v < RAW[0] - 1)
    a = aug[:, :, :, None]
    r = a[:, :, 0].float()
    u, v = u * r - a[:, :, 1].float(), v * r - a[:, :, 2].float()
    u = torch.where(a[:, :, 3] != 0, W - u, u)
    u, v = u - W / 2, v - H / 2
    ud, vd = u.double(), v.double()
    u, v = (a[:, :, 4] * ud + a[:, :, 5] * vd).float(), (-a[:, :, 5] * ud + a[:, :, 4] * vd).float()
    u, v = u + W / 2, v + H / 2
    ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
    iu, iv = u.clamp(0, W - 1).long(), v.clamp(0, H - 1).long()
    ok &= (iu % stride == 0) & (iv % stride == 0)
    return ok, (iv // stride) * (W // stride) + iu // stride, zc


def torch_labels(pts, lab, l2c, K, aug, bev, stride):
    """scatter_reduce_ formulation: int64 keys (value bits << 32 | index), 'amin' for the cameras, 'amax' for the BEV."""
    B, M = lab.shape
    N = l2c.shape[1]
    h, w = FINAL[0] // stride, FINAL[1] // stride
    idx = torch.arange(M, device=pts.device)
    ok, cell, depth = project_torch(pts, l2c, K, aug, stride)
    empty = torch.iinfo(torch.int64).max
    key = torch.where(ok, (depth.view(torch.int32).long() << 32) | idx, empty)      # depth > 0: the bits order as ints
    keys = torch.full((B, N, h * w), empty, dtype=torch.int64, device=pts.device)
    keys.scatter_reduce_(2, torch.where(ok, cell, 0), key, "amin")
    hit = keys != empty
    cam_depth = torch.where(hit, (keys >> 32).int().view(torch.float32), 0.0).view(B, N, h, w)
    win = (keys & 0xFFFFFFFF).clamp(max=M - 1)
    cam_seg = torch.where(hit, lab[:, None].expand(B, N, M).gather(2, win) & 0xFF, 0).view(B, N, h, w)
    size = bev["size"]
    nx, ny = int((bev["x_bound"][1] - bev["x_bound"][0]) / size), int((bev["y_bound"][1] - bev["y_bound"][0]) / size)
    cx = (pts[..., 0].double() - (bev["x_bound"][0] - size / 2.0)) / size
    cy = (pts[..., 1].double() - (bev["y_bound"][0] - size / 2.0)) / size
    z = pts[..., 2]
    ok = (cx > 1) & (cx < nx - 1) & (cy > 1) & (cy < ny - 1) & (z > bev["z_bound"][0]) & (z < bev["z_bound"][1])
    zb = z.view(torch.int32).long()
    ordered = torch.where(zb < 0, (~zb) & 0xFFFFFFFF, zb | 0x80000000)               # monotone, non-negative
    key = torch.where(ok, (ordered << 31) | (M - 1 - idx), 0)                       # (<< 31 keeps the key positive)
    cell = torch.where(ok, cy.clamp(0, ny - 1).long() * nx + cx.clamp(0, nx - 1).long(), 0)
    keys = torch.zeros(B, ny * nx, dtype=torch.int64, device=pts.device)
    keys.scatter_reduce_(1, cell, key, "amax")
    mask = keys != 0
    win = (M - 1 - (keys & 0x7FFFFFFF)).clamp(0, M - 1)
    bev_seg = torch.where(mask, lab.gather(1, win) & 0xFF, 0).view(B, 1, 1, ny, nx)
    bev_height = torch.where(mask, z.gather(1, win), 0.0).view(B, 1, 1, ny, nx)
    return cam_depth, cam_seg, cam_depth > 0, bev_seg, bev_height, mask.view(B, 1, 1, ny, nx)


def numpy_labels(pts, lab, l2c, K, aug, bev, stride):
    """Sort and assign on the host, one sample: what the loader's worker does per item."""
    H, W = FINAL
    h, w = H // stride, W // stride
    f32 = np.float32
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    maps = []
    for n in range(l2c.shape[0]):
        m, k, a = l2c[n], K[n], aug[n]
        with np.errstate(all="ignore"):
            xc, yc, zc = (m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(3))
            den = k[2, 0] * xc + k[2, 1] * yc + k[2, 2] * zc
            u, v = (k[0, 0] * xc + k[0, 1] * yc + k[0, 2] * zc) / den, (k[1, 0] * xc + k[1, 1] * yc + k[1, 2] * zc) / den
            ok = (zc > 0) & (u > 1) & (u < f32(RAW[1] - 1)) & (v > 1) & (v < f32(RAW[0] - 1))
            u, v = u * f32(a[0]) - f32(a[1]), v * f32(a[0]) - f32(a[2])
            if a[3]:
                u = f32(W) - u
            u, v = u - f32(W / 2), v - f32(H / 2)
            ud, vd = u.astype(np.float64), v.astype(np.float64)
            u, v = (a[4] * ud + a[5] * vd).astype(f32) + f32(W / 2), (-a[5] * ud + a[4] * vd).astype(f32) + f32(H / 2)
            ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
        i = np.flatnonzero(ok)
        iu, iv = u[i].astype(np.int64), v[i].astype(np.int64)
        on = (iu % stride == 0) & (iv % stride == 0)
        i, cell = i[on], (iv[on] // stride) * w + iu[on] // stride
        order = np.argsort(-zc[i], kind="stable")                   # far first: the nearest is written last
        depth, seg = np.zeros(h * w, f32), np.zeros(h * w, np.int64)
        depth[cell[order]], seg[cell[order]] = zc[i][order], lab[i][order] & 0xFF
        maps.append((depth, seg))
    size = bev["size"]
    nx, ny = int((bev["x_bound"][1] - bev["x_bound"][0]) / size), int((bev["y_bound"][1] - bev["y_bound"][0]) / size)
    cx = (x.astype(np.float64) - (bev["x_bound"][0] - size / 2.0)) / size
    cy = (y.astype(np.float64) - (bev["y_bound"][0] - size / 2.0)) / size
    ok = (cx > 1) & (cx < nx - 1) & (cy > 1) & (cy < ny - 1) & (z > f32(bev["z_bound"][0])) & (z < f32(bev["z_bound"][1]))
    i = np.flatnonzero(ok)
    order = np.argsort(z[i], kind="stable")
    cell = (cy[i].astype(np.int64) * nx + cx[i].astype(np.int64))[order]
    seg, height = np.zeros(ny * nx, np.int64), np.zeros(ny * nx, f32)
    seg[cell], height[cell] = lab[i][order] & 0xFF, z[i][order]
    return maps, seg, height


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for side in (256, 200):
        for M in (34720, 300000):
            for B in (1, 8):
                pts, lab, counts, l2c, K, aug, bev = make_inputs(B, M, side, dev)
                host = [t[0].cpu().numpy() for t in (pts, lab, l2c, K, aug)]
                for stride in (1, 4):
                    kw = dict(lidar2cam=l2c, intrins=K, aug=aug, final_dim=FINAL, raw_dim=RAW, stride=stride, bev=bev)
                    out = L.lidar_labels(pts, lab, counts=counts, **kw)
                    fn = lambda: L.lidar_labels(pts, lab, counts=counts, out=out, **kw)
                    ref = torch_labels(pts, lab, l2c, K, aug, bev, stride)
                    got = (out.cam_depth, out.cam_seg, out.cam_fg, out.bev_seg, out.bev_height, out.bev_mask)
                    equal = all(torch.equal(a, b) for a, b in zip(got, ref))
                    atomics = int(project_torch(pts, l2c, K, aug, stride)[0].sum()) + int(torch_bev_hits(pts, bev))
                    t0 = time.perf_counter()
                    numpy_labels(*host, bev, stride)
                    numpy_us = (time.perf_counter() - t0) * 1e6
                    hip_us = timed(fn, args.iters)
                    row = dict(bev=side, points=M, B=B, stride=stride, hip_us=round(hip_us, 1),
                               graph_us=round(timed_graph(fn, args.iters), 1),
                               torch_us=round(timed(lambda: torch_labels(pts, lab, l2c, K, aug, bev, stride),
                                                    max(args.iters // 5, 5), warmup=2), 1),
                               numpy_us_per_sample=round(numpy_us, 0), torch_equal=equal, atomics=atomics,
                               scatter_bytes_est=atomics * 64, scatter_gbs_est=round(atomics * 64 / hip_us / 1e3, 1),
                               written_cam=int(out.cam_fg.sum()), written_bev=int(out.bev_mask.sum()))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


def torch_bev_hits(pts, bev):
    size = bev["size"]
    nx, ny = int((bev["x_bound"][1] - bev["x_bound"][0]) / size), int((bev["y_bound"][1] - bev["y_bound"][0]) / size)
    cx = (pts[..., 0].double() - (bev["x_bound"][0] - size / 2.0)) / size
    cy = (pts[..., 1].double() - (bev["y_bound"][0] - size / 2.0)) / size
    z = pts[..., 2]
    return ((cx > 1) & (cx < nx - 1) & (cy > 1) & (cy < ny - 1) & (z > bev["z_bound"][0]) & (z < bev["z_bound"][1])).sum()


if __name__ == "__main__":
    main()
