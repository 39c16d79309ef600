"""Time the rgb loss: MultiTaskLoss's torch expression (smooth-L1 + 1 - ms_ssim) against ops.rgb_loss (vamp_rgb_loss_*).

    python tools/time_rgb_loss.py [--rounds 7] [--iters 20] [--json out.json] [--step]

Shapes of cfg-A: [N, 3, 256, 704] with N = 6 (batch 1) and N = 48 (batch 8), a textured label plus noise.  Each entry is
loss + backward to the prediction:
  torch          the expression and autograd, eager
  torch graph    the same captured in a CUDA graph, replayed
  device         ops.rgb_loss (six launches forward, five backward), eager
  device graph   the same captured, replayed
The candidates are timed in alternation, `rounds` rounds of `iters` calls each between device events; the table gives
the median round in microseconds per call.  `device_graph_gbps` is the traffic the loss cannot avoid (two images
read, one gradient written: 12 bytes per element) over the replayed device time: a rate for the whole path, not a
kernel's share of the memory bandwidth.  The split follows: forward and backward on their own through the C ABI, each
replayed from a graph of ten calls, and, where the profiler reports kernels, every launch of one forward + backward
in launch order (fwd scale 0 .. 4, finish, bwd scale 4 .. 0), the median of `iters` profiled calls.  --step adds
multitask_step at cfg-A, batch 1 (R50, bf16 autocast, AdamW, detection targets and loss on the device) with
MultiTaskLoss(rgb_loss="host") against rgb_loss="device", the median of 8 alternated steps in milliseconds.
Needs the GPU.
"""
import argparse
import json
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, ops  # noqa: E402
from vampire_amd import multitask as M  # noqa: E402
from vampire_amd._tensors import _stream  # noqa: E402
from vampire_amd.config import CFG_A  # noqa: E402

LAUNCHES = [f"fwd_scale{s}" for s in range(5)] + ["finish"] + [f"bwd_scale{s}" for s in range(4, -1, -1)]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternated(fns, rounds, iters):
    """{name: median over the rounds of microseconds per call}, the candidates taking turns inside every round."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return {k: round(sorted(v)[len(v) // 2], 1) for k, v in times.items()}


def captured(fn, calls=1):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    return g


def make_case(N, H, W, dev):
    g = torch.Generator().manual_seed(1)
    yy, xx = torch.linspace(0, 1, H)[:, None], torch.linspace(0, 1, W)[None, :]
    target = ((0.5 + 0.25 * torch.sin(9 * xx + 5 * yy))[None, None] + 0.15 * torch.rand(N, 3, H, W, generator=g)).clamp(0, 1)
    pred = (target + 0.2 * torch.randn(N, 3, H, W, generator=g)).clamp(0, 1)
    return pred.to(dev).requires_grad_(True), target.to(dev)


def abi_split(pred, target, rounds, iters):
    """forward / backward on their own through the C ABI, each replayed from a graph of ten calls."""
    dev = pred.device
    N, Cn, H, W = pred.shape
    d = _capi.VampRgbLossDesc(N, Cn, H, W, 1.0, 0.01, 0.03)
    vamp = _capi.checked()
    nbytes = vamp.vamp_rgb_loss_workspace_bytes(d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss, terms, vals = torch.empty((), device=dev), torch.empty(2, device=dev), torch.empty(N, 5, device=dev)
    one, grad, x = torch.ones((), device=dev), torch.empty_like(pred), pred.detach()
    fns = {
        "forward": lambda: vamp.vamp_rgb_loss_forward(d, x, target, loss, terms, vals, ws, ws.numel(), _stream()),
        "backward": lambda: vamp.vamp_rgb_loss_backward(d, x, target, one, grad, ws, ws.numel(), _stream()),
    }
    fns["forward"]()
    graphs = {k: captured(fn, calls=10) for k, fn in fns.items()}
    res = alternated({k: g.replay for k, g in graphs.items()}, rounds, iters)
    out = {f"{k}_us": round(v / 10, 1) for k, v in res.items()}
    out["workspace_mb"] = round(nbytes / 2 ** 20, 1)
    return out


def launch_split(fn, iters):
    """{launch: median microseconds} of the eleven kernels of one forward + backward, from the profiler's kernel
    records in launch order; a string saying why when the profiler reports none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if "rgb_" in e.name and "kernel" in e.name and e.device_time > 0]
        evs.sort(key=lambda e: e.time_range.start)
        if len(evs) != iters * len(LAUNCHES):
            return f"not measured: the profiler reported {len(evs)} kernel records for {iters * len(LAUNCHES)} launches"
        out = {}
        for j, name in enumerate(LAUNCHES):
            v = sorted(evs[i * len(LAUNCHES) + j].device_time for i in range(iters))
            out[name] = round(v[len(v) // 2], 1)
        return out
    except Exception as e:  # noqa: BLE001
        return f"not measured: {type(e).__name__}: {str(e).splitlines()[0][:160]}"


def step_rows(dev, steps, warm):
    torch.manual_seed(0)
    bb, hd = M.reference_confs(CFG_A)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(CFG_A.sdf_bias)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    data = M.synthetic_batch(CFG_A, 1, seed=0, device=dev, num_points=30000, num_boxes=30)
    fns = {k: M.MultiTaskLoss(model, sdf_bias=CFG_A.sdf_bias, det_targets="device", det_loss="device", rgb_loss=k)
           for k in ("host", "device")}
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", action="store_true", help="also time multitask_step at cfg-A with rgb_loss host / device")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = CFG_A.final_dim
    rows = []
    for N in (6, 48):
        pred, target = make_case(N, H, W, dev)

        def torch_path(pred=pred, target=target):
            loss = (F.smooth_l1_loss(pred, target, reduction="none") + 1 - M.ms_ssim(pred, target)).mean()
            return torch.autograd.grad(loss, [pred])

        def device_path(pred=pred, target=target):
            return torch.autograd.grad(ops.rgb_loss(pred, target), [pred])

        fns = {"torch_us": torch_path, "device_us": device_path, "device_graph_us": captured(device_path).replay}
        try:
            fns["torch_graph_us"] = captured(torch_path).replay
            note = None
        except Exception as e:  # noqa: BLE001
            note = f"not capturable: {type(e).__name__}: {str(e).splitlines()[0][:160]}"
        res = alternated(fns, args.rounds, args.iters)
        must_move = 12 * pred.numel()
        row = dict(N=N, C=3, H=H, W=W, **res, must_move_mb=round(must_move / 1e6, 1),
                   device_graph_gbps=round(must_move / res["device_graph_us"] / 1e3, 1))
        if note:
            row["torch_graph"] = note
        with torch.no_grad():
            d_loss = ops.rgb_loss(pred.detach(), target)
            t_loss = (F.smooth_l1_loss(pred, target, reduction="none") + 1 - M.ms_ssim(pred, target)).mean()
        row["loss_device"], row["loss_torch"] = float(d_loss), float(t_loss)
        assert math.isfinite(row["loss_device"])
        row.update(abi_split(pred, target, args.rounds, args.iters))
        row["launches_us"] = launch_split(device_path, args.iters)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del fns
    if args.step:
        row = dict(step="multitask_step cfg-A B=1", **{f"rgb_loss_{k}_ms": v for k, v in step_rows(dev, 8, 3).items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
