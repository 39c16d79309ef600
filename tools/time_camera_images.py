"""Time the camera image transform (images.camera_images / vamp_camera_images) against two formulations of the same
loader step.

    python tools/time_camera_images.py [--iters 200] [--json profiles/camera_images.json]

Configurations: six 900 x 1600 uint8 frames per sample to 256 x 704 (cfg-B), B = 1 and 8, fp32 and bf16 output, with
train-mode augmentation values drawn as sample_ida_augmentation draws them (resize 0.386 .. 0.55, rotate -5.4 .. 5.4,
random flip; seeded), the plan made for resize_min 0.386.
  hip_us     the call with out= buffers, device events around `iters` back-to-back calls
  graph_us   the same captured in a graph, ten calls per graph, replayed
  torch_us   a torch formulation on the same GPU, fp32 output only: per camera F.interpolate(mode="bicubic",
             antialias=True) of the float frame, rounded and clamped, copied into the crop window, flipped,
             grid_sample(mode="nearest") on a grid made beforehand (as the plan is), then the normalisation.  It is
             NOT bit-exact (float taps, no uint8 image between the passes, a float rotation): torch_max_u8_diff is its
             worst difference from the kernels' uint8 image, torch_u8_differing the share of bytes that differ.
  pillow_us_per_sample   the reference's own chain on the host for one sample (six frames: Pillow's resize, crop,
             transpose, rotate, then the numpy normalisation), where Pillow is importable; otherwise null and
             pillow = "absent".  pillow_equal: whether its uint8 images equal the kernels'.
Bytes: need_bytes is what the operation has to move at least -- the raw pixels under the crop windows' tap footprints,
read once, plus the output, written once; moved_bytes adds the uint8 staging image, written by the first kernel and
read by the second.  need_gbs / moved_gbs put them over the replayed time; roofline_share is moved_gbs over 8 TB/s.
No ratio is fixed in advance; the rows are what was measured.  Needs the GPU.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import images as I  # noqa: E402

RAW, FINAL = (900, 1600), (256, 704)
N_CAMS = 6
RESIZE_LIM, BOT_PCT_LIM, ROT_LIM = (0.386, 0.55), (0.0, 0.0), (-5.4, 5.4)
HBM_GBS = 8000.0


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


def train_augs(B, seed):
    rng = np.random.default_rng(seed)
    H, W = FINAL
    rows = []
    for _ in range(B):
        row = []
        for _ in range(N_CAMS):
            resize = float(rng.uniform(*RESIZE_LIM))
            new_w, new_h = int(RAW[1] * resize), int(RAW[0] * resize)
            y0 = int((1 - rng.uniform(*BOT_PCT_LIM)) * new_h) - H
            x0 = int(rng.uniform(0, max(0, new_w - W)))
            row.append((resize, (new_w, new_h), (x0, y0, x0 + W, y0 + H), bool(rng.integers(0, 2)),
                        float(rng.uniform(*ROT_LIM))))
        rows.append(row)
    return rows


def raw_frames(B, dev, seed):
    """Smooth gradients with noise on top: what a JPEG frame's statistics look like to a resampler."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    low = torch.rand(B * N_CAMS, 3, 30, 50, generator=g) * 255
    img = F.interpolate(low, size=RAW, mode="bilinear", align_corners=False) + torch.randn(B * N_CAMS, 3, *RAW, generator=g) * 12
    return img.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).reshape(B, N_CAMS, *RAW, 3).contiguous().to(dev)


def footprint_bytes(plan):
    """Raw bytes under the tap windows of every camera's crop window."""
    total = 0
    for b in range(plan.B):
        for n in range(plan.N):
            cc, rc = plan.col_count[b, n], plan.row_count[b, n]
            cf, rf = plan.col_first[b, n], plan.row_first[b, n]
            if (cc > 0).any() and (rc > 0).any():
                w = int((cf + cc)[cc > 0].max() - cf[cc > 0].min())
                h = int((rf + rc)[rc > 0].max() - rf[rc > 0].min())
                total += w * h * 3
    return total


def torch_grids(augs, dev):
    """The nearest-neighbour sampling grid of every camera's rotation, normalised for grid_sample (made beforehand)."""
    H, W = FINAL
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    grids = []
    for row in augs:
        for *_, rotate in row:
            a = -math.radians(rotate % 360.0)
            c, s = math.cos(a), math.sin(a)
            x, y = xs + 0.5 - W / 2, ys + 0.5 - H / 2
            sx, sy = c * x + s * y + W / 2, -s * x + c * y + H / 2
            grids.append(torch.stack([sx / W * 2 - 1, sy / H * 2 - 1], -1).float())
    return torch.stack(grids).view(len(augs), N_CAMS, H, W, 2).to(dev)


def torch_images(raw, augs, grids, mean, std_inv, out, out_u8=None):
    H, W = FINAL
    for b, row in enumerate(augs):
        for n, (_resize, (new_w, new_h), crop, flip, _rotate) in enumerate(row):
            x = raw[b, n].permute(2, 0, 1)[None].float()
            r = F.interpolate(x, size=(new_h, new_w), mode="bicubic", antialias=True, align_corners=False)
            r = r.round().clamp(0, 255)
            x0, y0 = crop[0], crop[1]
            win = torch.zeros(1, 3, H, W, device=raw.device)
            xa, xb, ya, yb = max(x0, 0), min(x0 + W, new_w), max(y0, 0), min(y0 + H, new_h)
            win[:, :, ya - y0:yb - y0, xa - x0:xb - x0] = r[:, :, ya:yb, xa:xb]
            if flip:
                win = win.flip(-1)
            rot = F.grid_sample(win, grids[b, n][None], mode="nearest", padding_mode="zeros", align_corners=False)
            if out_u8 is not None:
                out_u8[b, n] = rot[0].permute(1, 2, 0).to(torch.uint8)
            out[b, n] = (rot[0].flip(0) - mean) * std_inv
    return out


def pillow_sample(raw, augs_row, mean, std_inv):
    from PIL import Image
    outs, u8s = [], []
    for n, (_resize, dims, crop, flip, rotate) in enumerate(augs_row):
        img = Image.fromarray(raw[n]).resize(dims).crop(crop)
        if flip:
            img = img.transpose(method=Image.FLIP_LEFT_RIGHT)
        u8 = np.array(img.rotate(rotate))
        u8s.append(u8)
        outs.append(((u8[..., ::-1].astype(np.float32) - mean) * std_inv).transpose(2, 0, 1))
    return np.stack(outs), np.stack(u8s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    try:
        import PIL
        pillow = PIL.__version__
    except ImportError:
        pillow = "absent"
    mean = np.float32(I.IMG_MEAN)
    std_inv = (1.0 / np.float64(I.IMG_STD)).astype(np.float32)
    t_mean, t_std_inv = (torch.from_numpy(v).view(3, 1, 1).to(dev) for v in (mean, std_inv))
    H, W = FINAL
    rows = []
    for B in (1, 8):
        augs = train_augs(B, seed=B)
        raw = raw_frames(B, dev, seed=B)
        plan = I.plan_camera_images(augs, RAW, FINAL, resize_min=RESIZE_LIM[0]).to(dev)
        grids = torch_grids(augs, dev)
        ref, ref_u8 = I.camera_images(raw, plan, out_u8=True)
        t_out, t_u8 = torch.empty_like(ref), torch.empty_like(ref_u8)
        torch_images(raw, augs, grids, t_mean, t_std_inv, t_out, t_u8)
        diff = (t_u8.int() - ref_u8.int()).abs()
        torch_us = timed(lambda: torch_images(raw, augs, grids, t_mean, t_std_inv, t_out), max(args.iters // 10, 5), warmup=2)
        pillow_us, pillow_equal = None, None
        if pillow != "absent":
            host = raw[0].cpu().numpy()
            pillow_sample(host, augs[0], mean, std_inv)
            t0 = time.perf_counter()
            for _ in range(3):
                p_out, p_u8 = pillow_sample(host, augs[0], mean, std_inv)
            pillow_us = (time.perf_counter() - t0) / 3 * 1e6
            pillow_equal = bool(np.array_equal(p_u8, ref_u8[0].cpu().numpy())
                                and np.array_equal(p_out.view(np.int32), ref[0].cpu().numpy().view(np.int32)))
        raw_read = footprint_bytes(plan)
        stage = B * N_CAMS * H * W * 3
        for dtype in (torch.float32, torch.bfloat16):
            out = torch.empty(B, N_CAMS, 3, H, W, dtype=dtype, device=dev)
            fn = lambda: I.camera_images(raw, plan, dtype=dtype, out=out)
            fn()
            hip_us = timed(fn, args.iters)
            graph_us = timed_graph(fn, args.iters)
            need = raw_read + out.numel() * out.element_size()
            moved = need + 2 * stage
            row = dict(B=B, dtype=str(dtype).replace("torch.", ""), hip_us=round(hip_us, 1), graph_us=round(graph_us, 1),
                       torch_us=round(torch_us, 1) if dtype == torch.float32 else None,
                       torch_max_u8_diff=int(diff.max()), torch_u8_differing=round(float((diff > 0).float().mean()), 4),
                       pillow=pillow, pillow_us_per_sample=None if pillow_us is None else round(pillow_us, 0),
                       pillow_equal=pillow_equal, need_bytes=need, moved_bytes=moved,
                       need_gbs=round(need / graph_us / 1e3, 1), moved_gbs=round(moved / graph_us / 1e3, 1),
                       roofline_share=round(moved / graph_us / 1e3 / HBM_GBS, 4), foot=(plan.foot_h, plan.foot_w))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
