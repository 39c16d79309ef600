#!/usr/bin/env python3
"""Time the 2-D bilinear resizes between render and losses on the GPU: resize2d.hip against aten's F.interpolate.

Shapes: the pack of the three rendered camera maps (rgb 3, seg logits 18, depth 1 channels of 6 cameras, 64x176 ->
256x704: cfg-A and cfg-B share it) at batch 1 and 8, and cfg-A's 0.5x resize of the BEV feature (80 channels, 256^2 ->
128^2).  Forward and forward + backward, eager and replayed from a graph; the worst error of both paths against the
oracle of tests/test_resize2d.py (fp32 taps, float64 sums) at batch 1.  Writes profiles/resize2d.json."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from vampire_amd.layers import resize_bilinear2d_pack  # noqa: E402

CASES = [("camera maps cfg-A/B b1", [(1, 6, 3, 64, 176), (1, 6, 18, 64, 176), (1, 6, 1, 64, 176)], (256, 704)),
         ("camera maps cfg-A/B b8", [(8, 6, 3, 64, 176), (8, 6, 18, 64, 176), (8, 6, 1, 64, 176)], (256, 704)),
         ("bev feature cfg-A b1", [(1, 80, 256, 256)], (128, 128)),
         ("bev feature cfg-A b8", [(8, 80, 256, 256)], (128, 128))]


def hip(xs, size):
    return resize_bilinear2d_pack(xs, size)


def aten(xs, size):
    return [F.interpolate(x.flatten(0, -3)[None], size, mode="bilinear", align_corners=True)[0]
            .reshape(x.shape[:-2] + size) for x in xs]


def time_us(fn, n):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def replayed(make_fn, xs):
    """`make_fn(leaves)()` captured on one side stream and returned as its replay.  The leaves are made on that stream:
    capturing a backward on leaves that an eager backward on the default stream had used before ended this tool in a
    segmentation fault once (supposed cause: the default stream drawn into the capture)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn = make_fn([x.detach().clone().requires_grad_(True) for x in xs])
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--only", default="", help="time the cases whose name contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resize2d.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool times the MI355X kernels"
    dev = torch.device("cuda:0")
    import test_resize2d as T
    gen = torch.Generator().manual_seed(0)
    rows = []
    for name, shapes, size in CASES:
        if args.only not in name:
            continue
        xs = [torch.randn(s, generator=gen).to(dev).requires_grad_(True) for s in shapes]
        gs = [torch.randn(s[:-2] + size, generator=gen).to(dev) for s in shapes]
        row = dict(case=name, shapes=shapes, size=size,
                   bytes_each_way=sum(x.numel() + g.numel() for x, g in zip(xs, gs)) * 4)
        for path, f in (("hip", hip), ("aten", aten)):
            fwd = lambda leaves: lambda: f([x.detach() for x in leaves], size)
            both = lambda leaves: lambda: torch.autograd.grad(f(leaves, size), leaves, gs)
            row[path] = dict(forward_us=time_us(fwd(xs), args.iters), forward_backward_us=time_us(both(xs), args.iters),
                             forward_graph_us=time_us(replayed(fwd, xs), args.iters),
                             forward_backward_graph_us=time_us(replayed(both, xs), args.iters))
            if shapes[0][0] == 1:
                ys, gins = f(xs, size), torch.autograd.grad(f(xs, size), xs, gs)
                ef = eb = 0.0
                for x, g, y, gin in zip(xs, gs, ys, gins):
                    flat = lambda t: t.detach().flatten(0, -3).cpu().numpy()
                    ref, bound = T.oracle_forward(flat(x), *size)
                    rg, bg = T.oracle_backward(flat(g), *x.shape[-2:])
                    ef, eb = max(ef, T.worst(flat(y), ref, bound)[0]), max(eb, T.worst(flat(gin), rg, bg)[0])
                row[path].update(forward_max_err=ef, backward_max_err=eb)
        rows.append(row)
        print(json.dumps(row), flush=True)
    result = dict(device=torch.cuda.get_device_name(0), iters=args.iters, cases=rows)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    for r in rows:
        print("%-24s  fwd+bwd eager hip %7.1f us aten %7.1f us | graph hip %7.1f us aten %7.1f us | fwd graph hip %6.1f aten %6.1f"
              % (r["case"], r["hip"]["forward_backward_us"], r["aten"]["forward_backward_us"],
                 r["hip"]["forward_backward_graph_us"], r["aten"]["forward_backward_graph_us"],
                 r["hip"]["forward_graph_us"], r["aten"]["forward_graph_us"]))


if __name__ == "__main__":
    main()
