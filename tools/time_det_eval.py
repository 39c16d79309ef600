"""Time detection scoring: DetEvaluator.update (vamp_det_eval_update) against the host path a user had before it.

    python tools/time_det_eval.py [--iters 100] [--json out.json] [--only B]

The DetResult width of cfg-A's head (six tasks x post_max_size 83 = 498 rows, all filled), 40 ground-truth boxes per
sample over the ten classes, B = 1 and 8.  Per row, the median of 7 rounds that alternate the three measurements:
  host    DetResult.to_list() (the synchronisation) and the per-batch matching of the tests' float64 oracle in Python
  eager   DetEvaluator.update with packed ground truth, device events around `iters` back-to-back calls
  graph   the same call captured in a CUDA graph, ten calls per graph, replayed
and `compute_ms`: DetEvaluator.compute() on 1000 accumulated samples (host clock; it ends in the one synchronisation).
Times in microseconds per update.  Needs the GPU.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_det_eval as T  # noqa: E402  (the scenes and the oracle)
from vampire_amd import metrics  # noqa: E402
from vampire_amd import multitask as M  # noqa: E402

WIDTH, NUM_GT, ROUNDS = 498, 40, 7


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


def make_batch(B, dev, seed=0):
    rng = np.random.default_rng(seed)
    samples = [T.random_scene(rng, NUM_GT, WIDTH, list(range(len(M.CLASSES))), score_levels=128) for _ in range(B)]
    pad = torch.nn.utils.rnn.pad_sequence
    gb, gl, ga = T.gt_lists(samples, dev)
    gt = (pad(gb, batch_first=True), pad(gl, batch_first=True, padding_value=-1), pad(ga, batch_first=True, padding_value=-1))
    return samples, T.det_result(samples, WIDTH, dev), gt


def host_path(det, gt):
    """What a user could do before: bring the detections to the host and match them there."""
    gb, gl, ga = (x.cpu().numpy() for x in gt)
    samples = [T.sample(bx.cpu().numpy(), sc.float().cpu().numpy(), lb.cpu().numpy(), gb[b], gl[b], ga[b])
               for b, (bx, sc, lb) in enumerate(det.to_list())]
    return T.o_match(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--json", default=None)
    ap.add_argument("--only", default=None, help="B: one row, the device update alone (for a profiler run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for B in ([int(args.only)] if args.only else [1, 8]):
        _, det, gt = make_batch(B, dev)
        reps = max(args.iters // 10, 5)
        ev = metrics.DetEvaluator(M.CLASSES, B * (max(args.iters, 10 * reps) + 64), WIDTH, dev)
        update = lambda: ev.update(det, *gt)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                update()
        torch.cuda.current_stream().wait_stream(s)
        ev.reset()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(10):
                update()
        eager, graph, host = [], [], []
        for _ in range(1 if args.only else ROUNDS):
            ev.reset()
            eager.append(timed(update, args.iters))
            ev.reset()
            graph.append(timed(g.replay, reps, warmup=3) / 10)
            if not args.only:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host_path(det, gt)
                host.append((time.perf_counter() - t0) * 1e6)
        assert int(ev.state.state[1:5].sum()) == 0, "an update was dropped or counted an error"
        row = dict(B=B, width=WIDTH, gt_per_sample=NUM_GT, eager_us=round(statistics.median(eager), 1),
                   graph_us=round(statistics.median(graph), 1))
        if host:
            row["host_us"] = round(statistics.median(host), 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if not args.only:
        _, det, gt = make_batch(8, dev, seed=1)
        ev = metrics.DetEvaluator(M.CLASSES, 1000, WIDTH, dev)
        times = []
        for _ in range(ROUNDS):
            ev.reset()
            for _ in range(125):
                ev.update(det, *gt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ev.compute()
            times.append((time.perf_counter() - t0) * 1e3)
        row = dict(samples=1000, width=WIDTH, compute_ms=round(statistics.median(times), 1),
                   mAP=round(out["pts_bbox_NuScenes/mAP"], 4), NDS=round(out["pts_bbox_NuScenes/NDS"], 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
