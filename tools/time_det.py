"""Time detection post-processing: the host get_bboxes against get_bboxes_device (vamp_det_postprocess).

    python tools/time_det.py [--iters 100] [--json out.json]

Head shapes of cfg-A (128 x 128) and cfg-B (200 x 200), the six nuScenes tasks, max_num 500, B = 1 and 8, two
heatmaps: `worst` (every candidate above the threshold, dense and overlapping) and `sparse` (about 40 peaks per
task).  For circle, size-aware and rotate NMS:
  host    BEVDepthHead.get_bboxes (circle and size-aware only; the synchronising host path)
  eager   get_bboxes_device, device events around `iters` back-to-back calls (includes the launch cost)
  graph   the same call captured in a CUDA graph, ten calls per graph, replayed
Times in microseconds per call.  Needs the GPU.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from vampire_amd import multitask as M  # noqa: E402
from vampire_amd.config import CFG_A, CFG_B  # noqa: E402


def timed(fn, iters, warmup=10):
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


def make_head(cfg, kind):
    _, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    head = M.BEVDepthHead.__new__(M.BEVDepthHead)
    head.bbox_coder = M.CenterPointBBoxCoder(**hd["bbox_coder"])
    head.num_classes = [t["num_class"] for t in M.TASKS]
    head.norm_bbox = True
    head.test_cfg = dict(hd["test_cfg"], nms_type=kind, thresh_scale=[1.0] * 6)
    return head, hd["train_cfg"]["grid_size"][0] // 4


def make_preds(B, side, scene, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    preds = []
    for t in M.TASKS:
        shape = (B, t["num_class"], side, side)
        if scene == "worst":
            heat = torch.randn(shape, generator=g) * 1.5 + 1.0
        else:
            heat = torch.full(shape, -8.0)
            flat = heat.view(B, -1)
            for b in range(B):
                flat[b, torch.randint(0, flat.shape[1], (40,), generator=g)] = torch.rand(40, generator=g) * 6 - 1
        p = dict(heatmap=heat, reg=torch.rand(B, 2, side, side, generator=g),
                 height=torch.randn(B, 1, side, side, generator=g),
                 dim=torch.rand(B, 3, side, side, generator=g) * 3.7 - 1.2,
                 rot=torch.randn(B, 2, side, side, generator=g), vel=torch.randn(B, 2, side, side, generator=g))
        preds.append([{k: v.to(dev) for k, v in p.items()}])
    return preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="cfg,B,scene,kind: one row (for a profiler run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    combos = [(c, B, s, k) for c in ("A", "B") for B in (1, 8) for s in ("worst", "sparse")
              for k in ("circle", "size_aware_circle", "rotate")]
    if args.only:
        c, B, s, k = args.only.split(",")
        combos = [(c, int(B), s, k)]
    for cname, B, scene, kind in combos:
        head, side = make_head({"A": CFG_A, "B": CFG_B}[cname], kind)
        preds = make_preds(B, side, scene, dev)
        res = head.get_bboxes_device(preds)
        kept = int(res.counts.sum())
        row = dict(cfg=cname, side=side, B=B, scene=scene, nms=kind, kept=kept,
                   eager_us=round(timed(lambda: head.get_bboxes_device(preds, out=res), args.iters), 1),
                   graph_us=round(timed_graph(lambda: head.get_bboxes_device(preds, out=res), args.iters), 1))
        if kind != "rotate" and not args.only:
            row["host_us"] = round(timed(lambda: head.get_bboxes(preds), max(args.iters // 10, 3), warmup=2), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
