"""Time the segmentation loss: MultiTaskLoss's torch expression `_ce_lovasz(x[mask], y[mask])` against ops.seg_loss
(vamp_seg_loss_*), at the four call sites of the training step.

    python tools/time_seg_loss.py [--rounds 5] [--iters 5] [--json out.json] [--step] [--configs A1,B8]

Sites, with labels and masks from synthetic_batch(cfg, batch) and 3 randn logits in the memory layout the model hands
over: camera ([B, N, K, h, w] behind permute(0, 1, 3, 4, 2), mask depth > 0), bev ([B, K, oY, oX] behind a permute,
bev_mask), lidar (rows [sum of points, K], no mask), occupancy ([B, K, 200, 200, 16] behind a permute, mask_camera);
cfg-A batch 1 and cfg-B batch 8.  Each entry is loss + backward to the logits:
  torch          the expression and autograd, eager (the boolean-mask indexing synchronises: not capturable)
  device         ops.seg_loss, eager
  device graph   the same captured in a graph, replayed
The candidates are timed in alternation, `rounds` rounds of `iters` calls each between device events; the table gives
the median round in microseconds per call and the spread (min, max) of the rounds.  Errors: loss and gradient of both
paths against a float64 evaluation on the same device, each under its own permutation (the torch path's from the same op
sequence with a stable sort), the gradient's largest absolute difference over the oracle gradient's largest magnitude.
--step adds multitask_step at cfg-A, batch 1 (R50, bf16 autocast, AdamW, detection targets and loss on the device) with
MultiTaskLoss(seg_loss="host") against seg_loss="device", the median of 8 alternated steps in milliseconds.
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

from vampire_amd import losses, ops  # noqa: E402
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
        for _ in range(2):
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
    """{site: (logits view with requires_grad, labels, mask or None)} shaped like MultiTaskLoss's four calls."""
    data = M.synthetic_batch(cfg, batch, seed=0, device=dev, num_points=30000, num_boxes=4)
    K = cfg.num_classes
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *shape: (3.0 * torch.randn(*shape, generator=g, device=dev)).requires_grad_(True)
    seg_l, depth = data[7][:, 0], data[6][:, 0]
    B, N, h, w = seg_l.shape
    out = {"camera": (rnd(B, N, K, h, w).permute(0, 1, 3, 4, 2), seg_l, depth > 0)}
    bev_seg, bev_mask = data[8], data[10]
    out["bev"] = (rnd(B, K, *bev_seg.shape[-2:])[:, None, None].permute(0, 1, 2, 4, 5, 3), bev_seg, bev_mask)
    out["lidar"] = (rnd(sum(len(p) for p in data[12]), K), torch.cat(data[12], 0), None)
    occ_sem, mask_cam = data[16], data[19]
    out["occupancy"] = (rnd(B, K, *occ_sem.shape[1:]).permute(0, 2, 3, 4, 1), occ_sem, mask_cam)
    return out


def oracle(x, y, perm):
    """float64 CE + Lovasz and its gradient on compacted device tensors x [n, C], y [n] under `perm` [C, n]: the
    Jaccard steps in closed form from integer counts (seg_loss.hip's algebra).  Returns (loss, grad [n, C])."""
    n, Cn = x.shape
    p = F.softmax(x.double(), dim=1)
    fg = F.one_hot(y, Cn).double()
    d = fg - p
    f = fg.t().gather(1, perm)
    G = f.sum(1, keepdim=True)
    cum = f.cumsum(1)
    U = G + torch.arange(1, n + 1, device=x.device, dtype=torch.float64)[None] - cum
    delta = torch.where(f > 0, 1.0 / U, (G - cum) / ((U - 1.0) * U).clamp(min=1.0)) * (G > 0)
    present = (G > 0).sum().clamp(min=1)
    lv = (d.abs().t().gather(1, perm) * delta).sum() / present
    gp = torch.zeros_like(p.t()).scatter_(1, perm, -torch.sign(d.t().gather(1, perm)) * delta).t() / present
    grad = (p - fg) / n + p * (gp - (p * gp).sum(1, keepdim=True))
    return float(F.cross_entropy(x.double(), y) + lv), grad


def lovasz_stable(probas, labels):
    """multitask.lovasz_softmax's op sequence with a stable sort; also returns the permutation."""
    Cn = probas.shape[1]
    fg = F.one_hot(labels, Cn).to(probas.dtype).t().contiguous()
    present = fg.sum(1) > 0
    err, perm = (fg - probas.t()).abs().sort(dim=1, descending=True, stable=True)
    fgs = fg.gather(1, perm)
    gts = fgs.sum(1, keepdim=True)
    jac = 1.0 - (gts - fgs.cumsum(1)) / (gts + (1 - fgs).cumsum(1))
    jac = torch.cat([jac[:, :1], jac[:, 1:] - jac[:, :-1]], 1)
    return ((err * jac).sum(1) * present).sum() / present.sum().clamp(min=1), perm


def errors(x, y, m):
    """{loss / grad error of the device and of the torch path} against the float64 oracle, each under its own order."""
    Cn = x.shape[-1]
    flat, lab = x.detach().reshape(-1, Cn), y.reshape(-1).long()
    valid = torch.ones_like(lab, dtype=torch.bool) if m is None else m.reshape(-1)
    vidx = valid.nonzero()[:, 0]
    xc, yc = flat[vidx].contiguous(), lab[vidx]
    gerr = lambda a, ref: float((a.double() - ref).abs().max() / ref.abs().max())
    # device: the order from the sort window, mapped to compacted positions
    d, lx, ly, lm = losses._seg_inputs(flat, lab, valid, 1.0, 1.0)
    _, _, counts, _, _, perm = losses._seg_forward(d, lx, ly, lm, window=True)
    n = int(counts[0])
    pos = torch.full((flat.shape[0],), -1, dtype=torch.int64, device=x.device)
    pos[vidx] = torch.arange(n, device=x.device)
    o_loss, o_grad = oracle(xc, yc, pos[perm[:, :n].long()])
    del perm
    xg = flat.clone().requires_grad_(True)
    loss = ops.seg_loss(xg, lab, valid)
    g, = torch.autograd.grad(loss, [xg])
    out = dict(device_loss_err=abs(float(loss) - o_loss) / abs(o_loss), device_grad_err=gerr(g[vidx], o_grad))
    del o_grad, g
    xt = xc.clone().requires_grad_(True)
    lv, t_perm = lovasz_stable(F.softmax(xt, dim=1), yc)
    t_loss = F.cross_entropy(xt, yc) + lv
    tg, = torch.autograd.grad(t_loss, [xt])
    o_loss, o_grad = oracle(xc, yc, t_perm)
    out.update(torch_loss_err=abs(float(t_loss) - o_loss) / abs(o_loss), torch_grad_err=gerr(tg, o_grad))
    return {k: float(f"{v:.3e}") for k, v in out.items()}


def step_rows(dev, steps, warm):
    torch.manual_seed(0)
    bb, hd = M.reference_confs(CFG_A)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(CFG_A.sdf_bias)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    data = M.synthetic_batch(CFG_A, 1, seed=0, device=dev, num_points=30000, num_boxes=30)
    fns = {k: M.MultiTaskLoss(model, sdf_bias=CFG_A.sdf_bias, det_targets="device", det_loss="device", seg_loss=k)
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--configs", default="A1,B8", help="comma-separated cfg letter + batch, of A1 and B8")
    ap.add_argument("--no-errors", action="store_true", help="skip the float64 error table")
    ap.add_argument("--step", action="store_true", help="also time multitask_step at cfg-A with seg_loss host / device")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for name in args.configs.split(","):
        cfg, batch = {"A": CFG_A, "B": CFG_B}[name[0]], int(name[1:])
        for site, (x, y, m) in sites(cfg, batch, dev).items():

            def torch_path(x=x, y=y, m=m):
                loss = M._ce_lovasz(x, y) if m is None else M._ce_lovasz(x[m], y[m])
                return torch.autograd.grad(loss, [x])

            def device_path(x=x, y=y, m=m):
                return torch.autograd.grad(ops.seg_loss(x, y, m), [x])

            fns = {"torch_us": torch_path, "device_us": device_path, "device_graph_us": captured(device_path).replay}
            res = alternated(fns, args.rounds, args.iters)
            P, K = y.numel(), x.shape[-1]
            row = dict(config=name, site=site, P=P, C=K, valid=int(P if m is None else m.sum()))
            for k, (med, lo, hi) in res.items():
                row[k], row[k.replace("_us", "_spread_us")] = med, [lo, hi]
            with torch.no_grad():
                row["loss_device"] = float(ops.seg_loss(x.detach(), y, m))
                row["loss_torch"] = float(M._ce_lovasz(x, y) if m is None else M._ce_lovasz(x[m], y[m]))
            assert math.isfinite(row["loss_device"])
            del fns
            if not args.no_errors:
                row.update(errors(x, y, m))
            rows.append(row)
            print(json.dumps(row), flush=True)
            del x, y, m
            torch.cuda.empty_cache()
    if args.step:
        row = dict(step="multitask_step cfg-A B=1", **{f"seg_loss_{k}_ms": v for k, v in step_rows(dev, 8, 3).items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
