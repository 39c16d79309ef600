"""Time the masked regression losses: MultiTaskLoss's torch expressions (boolean-mask compaction + F.smooth_l1_loss /
squared-error mean) against ops.reg_losses (vamp_reg_loss_*), at the shapes of the four call sites of the training step.

    python tools/time_reg_loss.py [--rounds 7] [--iters 20] [--json out.json] [--configs A1,B8]

Sites, with labels and masks from synthetic_batch(cfg, batch) and randn predictions shaped as the model hands them
over: depth ([B, N, h, w], smooth-L1 where the depth label is > 0), height ([B, 1, 1, oY, oX], smooth-L1 under
bev_mask), sdf ([B x 30000 points], squared error against sdf_bias, no mask), density ([B, 200, 200, 16], squared
error under mask_camera plus under its complement), and `all`: the four together -- four torch expressions against
ONE pack; cfg-A batch 1 and cfg-B batch 8.  Each entry is loss + backward to the predictions:
  torch          the expression and autograd, eager (the boolean-mask indexing synchronises: not capturable)
  device         ops.reg_losses, eager
  device graph   the same captured in a graph, replayed
The candidates are warmed up and then timed in alternation, `rounds` rounds of `iters` calls each between device
events; the table gives the median round in microseconds per call and the spread (min, max) of the rounds.
`bytes` is what the pack has to move (forward: pred, target, mask; backward: the same and the gradient) and
`device_graph_gbps_warm` that over the replayed time.  Every call reads the same buffers again, so the cache state is
WARM: a working set below the 256 MB last-level cache (every row but `all` at cfg-B batch 8, 313 MB) can be served
from it, so these figures are no HBM rates.  Errors: loss and gradient of both paths against a float64
evaluation of the definition on the same device, the gradient's largest absolute difference over the oracle
gradient's largest magnitude.
Needs the GPU.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import ops  # noqa: E402
from vampire_amd import multitask as M  # noqa: E402
from vampire_amd.config import CFG_A, CFG_B  # noqa: E402


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def alternated(fns, rounds, iters):
    """{name: (median, min, max) over the rounds of microseconds per call}, the candidates taking turns."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, iters))
    return {k: (round(sorted(v)[len(v) // 2], 1), round(min(v), 1), round(max(v), 1)) for k, v in times.items()}


def captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def sites(cfg, batch, dev):
    """{site: RegTerm} shaped like the four regression terms of MultiTaskLoss; every pred requires a gradient."""
    data = M.synthetic_batch(cfg, batch, seed=0, device=dev, num_points=30000, num_boxes=4)
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda shape, scale=1.0: (scale * torch.randn(*shape, generator=g, device=dev)).requires_grad_(True)
    depth = data[6][:, 0]
    out = {"depth": ops.RegTerm(rnd(depth.shape, 20.0), depth, depth > 0, "smooth_l1", "set")}
    out["height"] = ops.RegTerm(rnd(data[9].shape, 3.0), data[9], data[10], "smooth_l1", "set")
    out["sdf"] = ops.RegTerm(rnd((sum(len(p) for p in data[11]),)), float(cfg.sdf_bias), None, "mse", "set")
    out["density"] = ops.RegTerm(rnd(data[17].shape), data[17], data[19], "mse", "both")
    return out


def host_term(t, dtype=None):
    """MultiTaskLoss's host expression of one term, optionally in another dtype (the oracle): (loss, its pred leaf)."""
    x = t.pred if dtype is None else t.pred.detach().to(dtype).requires_grad_(True)
    y = t.target.to(x.dtype) if torch.is_tensor(t.target) else None
    pick = lambda v, m: v if m is None else v[m]

    def expr(m):
        a, b = pick(x, m), t.target if y is None else pick(y, m)
        if t.kind == "mse":
            return ((a - b) ** 2).mean()
        return F.smooth_l1_loss(a, b if y is not None else torch.full_like(a, b))

    loss = expr(t.mask)
    if t.side == "both":
        loss = loss + expr(~t.mask)
    return loss, x


def errors(t):
    """{loss / grad error of the device and of the torch path} against the float64 evaluation on the device."""
    o_loss, x64 = host_term(t, torch.float64)
    o_grad, = torch.autograd.grad(o_loss, [x64])
    top = float(o_grad.abs().max())
    gerr = lambda a: float((a.double() - o_grad).abs().max()) / top
    rel = lambda a: abs(float(a.double()) - float(o_loss)) / abs(float(o_loss))
    d_loss = ops.reg_losses([t])[0]
    d_grad, = torch.autograd.grad(d_loss, [t.pred])
    t_loss, _ = host_term(t)
    t_grad, = torch.autograd.grad(t_loss, [t.pred])
    out = dict(device_loss_err=rel(d_loss), device_grad_err=gerr(d_grad), torch_loss_err=rel(t_loss),
               torch_grad_err=gerr(t_grad))
    return {k: float(f"{v:.3e}") for k, v in out.items()}


def pack_bytes(terms):
    """Bytes the pack has to move, forward + backward: pred twice, target twice, mask twice, the gradient once."""
    total = 0
    for t in terms:
        n, e = t.pred.numel(), t.pred.element_size()
        total += n * (2 * e + (8 if torch.is_tensor(t.target) else 0) + (2 if t.mask is not None else 0) + e)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--configs", default="A1,B8", help="comma-separated cfg letter + batch, of A1 and B8")
    ap.add_argument("--no-errors", action="store_true", help="skip the float64 error table")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reg_loss.py needs the GPU: nothing is measured without one")
    dev = torch.device("cuda:0")
    rows = []
    for name in args.configs.split(","):
        cfg, batch = {"A": CFG_A, "B": CFG_B}[name[0]], int(name[1:])
        terms = sites(cfg, batch, dev)
        for site, pack in list((k, [t]) for k, t in terms.items()) + [("all", list(terms.values()))]:
            preds = [t.pred for t in pack]

            def torch_path(pack=pack, preds=preds):
                return torch.autograd.grad(sum(host_term(t)[0] for t in pack), preds)

            def device_path(pack=pack, preds=preds):
                return torch.autograd.grad(ops.reg_losses(pack).sum(), preds)

            fns = {"torch_us": torch_path, "device_us": device_path, "device_graph_us": captured(device_path).replay}
            res = alternated(fns, args.rounds, args.iters)
            row = dict(config=name, site=site, n=sum(p.numel() for p in preds), bytes=pack_bytes(pack))
            for k, (med, lo, hi) in res.items():
                row[k], row[k.replace("_us", "_spread_us")] = med, [lo, hi]
            row["cache"], row["device_graph_gbps_warm"] = "warm", round(row["bytes"] / row["device_graph_us"] / 1e3, 1)
            with torch.no_grad():
                row["loss_device"] = [round(v, 6) for v in ops.reg_losses(pack).tolist()]
                row["loss_torch"] = [round(float(host_term(t)[0]), 6) for t in pack]
            assert all(math.isfinite(v) for v in row["loss_device"])
            del fns
            if not args.no_errors and len(pack) == 1:
                row.update(errors(pack[0]))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del terms
        torch.cuda.empty_cache()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
