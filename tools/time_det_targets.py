"""Time detection training targets: the host get_targets against get_targets_device (vamp_det_targets).

    python tools/time_det_targets.py [--iters 100] [--json out.json] [--step]

Train configurations of cfg-A (128 x 128 map) and cfg-B (200 x 200), the six nuScenes tasks, max_objs 500,
B = 1 and 8, 12 / 40 / 200 synthetic boxes per sample (synthetic_batch's generator):
  host    BEVDepthHead.get_targets on device tensors (the per-box host loop, its copies and synchronisations)
  list    get_targets_device on the per-sample lists (pad_sequence + the two launches), device events around
          `iters` back-to-back calls
  packed  the same on packed [B, M, 9] / [B, M] tensors
  graph   the packed call captured in a CUDA graph, ten calls per graph, replayed
Times in microseconds per call.  --step adds multitask_step at cfg-A, batch 1 (R50, bf16 autocast, AdamW), with
MultiTaskLoss(det_targets="host") against "device", alternated, in milliseconds per step.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def make_head(cfg, dev):
    torch.manual_seed(0)
    _, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    return M.BEVDepthHead(**hd).to(dev)


def boxes_of(cfg, B, n, dev):
    g = torch.Generator().manual_seed(n)
    lo, hi = cfg.x_bound_det[:2]
    boxes, labels = [], []
    for _ in range(B):
        xy = torch.rand(n, 2, generator=g) * (hi - lo) * 0.9 + lo * 0.9
        z = torch.rand(n, 1, generator=g) * 2 - 1.5
        dims = torch.rand(n, 3, generator=g) * torch.tensor([1.5, 3.5, 1.0]) + torch.tensor([0.6, 0.8, 1.0])
        yaw = (torch.rand(n, 1, generator=g) * 2 - 1) * 3.14159
        vel = torch.randn(n, 2, generator=g)
        boxes.append(torch.cat([xy, z, dims, yaw, vel], 1).to(dev))
        labels.append(torch.randint(0, 10, (n,), generator=g).to(dev))
    return boxes, labels


def step_rows(dev, steps, warm):
    torch.manual_seed(0)
    bb, hd = M.reference_confs(CFG_A)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(CFG_A.sdf_bias)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    data = M.synthetic_batch(CFG_A, 1, seed=0, device=dev, num_points=30000, num_boxes=30)
    fns = {k: M.MultiTaskLoss(model, sdf_bias=CFG_A.sdf_bias, det_targets=k) for k in ("host", "device")}
    for fn in fns.values():
        for _ in range(warm):
            M.multitask_step(model, fn, data, optimizer=opt)
    times = {k: [] for k in fns}
    for _ in range(steps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M.multitask_step(model, fn, data, optimizer=opt)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: round(sorted(v)[len(v) // 2], 2) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", action="store_true", help="also time multitask_step at cfg-A with host / device targets")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for cname in ("A", "B"):
        cfg = {"A": CFG_A, "B": CFG_B}[cname]
        head = make_head(cfg, dev)
        for B in (1, 8):
            for n in (12, 40, 200):
                boxes, labels = boxes_of(cfg, B, n, dev)
                packed_b = torch.nn.utils.rnn.pad_sequence(boxes, batch_first=True)
                packed_l = torch.nn.utils.rnn.pad_sequence(labels, batch_first=True, padding_value=-1)
                out = head.get_targets_device(packed_b, packed_l)
                row = dict(cfg=cname, side=out.fw, B=B, boxes=n,
                           list_us=round(timed(lambda: head.get_targets_device(boxes, labels), args.iters), 1),
                           packed_us=round(timed(lambda: head.get_targets_device(packed_b, packed_l, out=out),
                                                 args.iters), 1),
                           graph_us=round(timed_graph(lambda: head.get_targets_device(packed_b, packed_l, out=out),
                                                      args.iters), 1),
                           host_us=round(timed(lambda: head.get_targets(boxes, labels), 5, warmup=2), 1))
                rows.append(row)
                print(json.dumps(row), flush=True)
    if args.step:
        row = dict(step="multitask_step cfg-A B=1", **{f"{k}_ms": v for k, v in step_rows(dev, 8, 3).items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
