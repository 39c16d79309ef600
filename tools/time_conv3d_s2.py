#!/usr/bin/env python3
"""The stride-2 3x3x3 layers of the UNet in 16 bits: the HIP kernels (ops.conv3d_bf16_stride2) against MIOpen through
torch, in one process and one run -- MIOpen on NCDHW tensors (what autocast calls) and on channels_last_3d ones --
forward and forward + backward, bf16 and fp16, at the cfg-B layers (16->32 at 16x200x200, 32->32 at 8x100x100) and the
cfg-A ones (16->32 at 10x128x128, 32->32 at 5x64x64).  Then Unet3D(16, 16) forward + backward at cfg-B under both
autocasts with `SWITCHES.conv3d_s2` off and on.

The contenders of a row alternate round by round; a figure is the median of the rounds' means, the spread is the
rounds' min .. max.  A window is enqueued behind a long matrix product, so the figures are device time (these layers
take less time on the GPU than their launches take on the host).  The first line of each layer compares the two
outputs on the timed inputs.
usage: tools/time_conv3d_s2.py [--rounds R] [--reps N] [--no-unet]"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vampire_amd import backbone                                    # noqa: E402
from vampire_amd.ops import conv3d_bf16_stride2                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-unet", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "this tool times kernels on the GPU"
dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True
LAYERS = [("cfg-B conv1", 16, 32, (16, 200, 200)), ("cfg-B conv3", 32, 32, (8, 100, 100)),
          ("cfg-A conv1", 16, 32, (10, 128, 128)), ("cfg-A conv3", 32, 32, (5, 64, 64))]
CL = torch.channels_last_3d


_busy = torch.randn(8192, 8192, device=dev)


def mean_us(fn, reps):
    """Device time per call: an fp32 8192^3 product keeps the GPU busy while the host enqueues the whole window, so the
    calls run back to back and the events bracket the kernels, not the Python that launches them."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    _busy @ _busy
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def contest(fns, rounds, reps):
    """{name: (median, min, max)} of the rounds' mean times, the contenders alternating inside every round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            t[k].append(mean_us(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def show(tag, res, unit="us", scale=1.0):
    for k, (med, lo, hi) in res.items():
        print("%-34s %-28s %9.1f %s   (%.1f .. %.1f)" % (tag, k, med * scale, unit, lo * scale, hi * scale), flush=True)


print("rounds %d x reps %d; median of the rounds' means (min .. max)" % (args.rounds, args.reps))
for dt in (torch.bfloat16, torch.float16):
    name = "bf16" if dt == torch.bfloat16 else "fp16"
    for layer, cin, cout, vol in LAYERS:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(1, cin, *vol, device=dev, generator=g).to(dt)
        w = (torch.randn(cout, cin, 3, 3, 3, device=dev, generator=g) * 0.05).to(dt)
        ovol = [(n - 1) // 2 + 1 for n in vol]
        up = torch.randn(1, cout, *ovol, device=dev, generator=g).to(dt)
        xc, wc, uc = (t.contiguous(memory_format=CL) for t in (x, w, up))
        ref = F.conv3d(x.float(), w.float(), stride=2, padding=1)
        tag = "%s %s %d->%d %s" % (name, layer, cin, cout, "x".join(map(str, vol)))
        print("%-34s max |hip - fp32| %.3e   max |miopen - fp32| %.3e   max |ref| %.3e" % (
            tag, float((conv3d_bf16_stride2(x, w).float() - ref).abs().max()),
            float((F.conv3d(x, w, stride=2, padding=1).float() - ref).abs().max()), float(ref.abs().max())), flush=True)

        def runner(f, a, b, u, bwd):
            def run():
                aa, bb = a.detach().requires_grad_(bwd), b.detach().requires_grad_(bwd)
                y = f(aa, bb)
                if bwd:
                    y.backward(u)
            return run

        mi = lambda p, q: F.conv3d(p, q, stride=2, padding=1)          # noqa: E731
        for bwd in (False, True):
            res = contest({"hip": runner(conv3d_bf16_stride2, x, w, up, bwd), "miopen NCDHW": runner(mi, x, w, up, bwd),
                           "miopen channels_last_3d": runner(mi, xc, wc, uc, bwd)}, args.rounds, args.reps)
            show(tag + (" fwd+bwd" if bwd else " fwd"), res)

if not args.no_unet:
    x0 = torch.randn(1, 16, 16, 200, 200, device=dev)
    torch.manual_seed(0)
    net = backbone.Unet3D(16, 16).to(dev)
    x0.requires_grad_(True)
    for dt in (torch.bfloat16, torch.float16):
        def stepper(on):
            def step():
                backbone.SWITCHES.conv3d_s2 = on
                net.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=dt):
                    y = net(x0)
                y.float().mean().backward()
            return step
        res = contest({"conv3d_s2 off (MIOpen)": stepper(False), "conv3d_s2 on (HIP)": stepper(True)}, args.rounds, 5)
        show("Unet3D cfg-B %s autocast fwd+bwd" % ("bf16" if dt == torch.bfloat16 else "fp16"), res, "ms", 1e-3)
