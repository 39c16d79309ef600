"""Time the detection loss: the torch BEVDepthHead.loss against loss_device (vamp_det_loss_*).

    python tools/time_det_loss.py [--rounds 7] [--iters 20] [--json out.json] [--torch-graph] [--step]

Train configurations of cfg-A (128 x 128 map) and cfg-B (200 x 200), the six nuScenes tasks, max_objs 500,
B = 1 and 8, 40 synthetic boxes per sample, targets from get_targets_device, random fp32 head outputs.  Each entry
is loss + backward to the prediction tensors:
  torch         BEVDepthHead.loss on cloned dicts (it replaces their heatmaps) and autograd, eager
  device        loss_device (counts, forward, backward: five launches), eager
  device graph  the same captured in a CUDA graph, replayed
  torch graph   (--torch-graph, in a second pass) the torch path captured and replayed, against the device graph
                again; loss runs on a stand-in head whose code weights were uploaded once (its per-call upload from
                host memory cannot be captured)
The candidates are timed in alternation, `rounds` rounds of `iters` calls each between device events; the table
gives the median round in microseconds per call.  The kernel split (counts / forward / backward through the C ABI,
replayed from a graph of ten calls) follows.  --step adds multitask_step at cfg-A, batch 1 (R50, bf16 autocast, AdamW) with
MultiTaskLoss(det_targets="device", det_loss="host") against det_loss="device", the median of 8 alternated steps
in milliseconds.  Needs the GPU.
"""
import argparse
import json
import os
import sys
import time
import types
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, evaluation  # noqa: E402
from vampire_amd import multitask as M  # noqa: E402
from vampire_amd._tensors import _stream  # noqa: E402
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


def make_case(cfg, B, dev, boxes=40):
    torch.manual_seed(0)
    _, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    head = M.BEVDepthHead(**hd).to(dev)
    batch = M.synthetic_batch(cfg, B, seed=1, device=dev, num_points=10, num_boxes=boxes)
    tg = head.get_targets_device(batch[4], batch[5])
    g = torch.Generator().manual_seed(2)
    preds = []
    for n in tg.ncls:
        p = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2, "heatmap": n}
        preds.append([{k: (torch.randn(B, c, tg.fh, tg.fw, generator=g) * (3 if k == "heatmap" else 1)
                           - (2.19 if k == "heatmap" else 0)).to(dev).requires_grad_(True) for k, c in p.items()}])
    return head, tg, preds


def kernel_split(head, tg, preds, rounds, iters):
    """counts / forward / backward on their own through the C ABI, each replayed from a graph of ten calls."""
    dev = tg.heat.device
    T, B = len(tg.ncls), tg.anno.shape[1]
    d = _capi.VampDetLossDesc()
    d.B, d.T, d.H, d.W = B, T, tg.fh, tg.fw
    for t, n in enumerate(tg.ncls):
        d.ncls[t] = n
    cw = head.train_cfg["code_weights"]
    d.code, d.max_objs, d.has_vel = len(cw), tg.anno.shape[2], 1
    for c, w in enumerate(cw):
        d.code_weights[c] = w
    d.loss_bbox_weight = head.loss_bbox_weight
    keys = ("heatmap", "reg", "height", "dim", "rot", "vel")
    rows = [[pd[0][k].detach() for k in keys] for pd in preds]
    grows = [[torch.empty_like(x) for x in r] for r in rows]
    table, gtable = evaluation._det_task_table(T, rows), evaluation._det_task_table(T, grows)
    vamp = _capi.checked()
    ws = torch.empty(vamp.vamp_det_loss_workspace_bytes(d), dtype=torch.uint8, device=dev)
    counts = torch.empty(T, 2, device=dev)
    loss, terms, one = torch.empty((), device=dev), torch.empty(T, 2, device=dev), torch.ones((), device=dev)
    fns = {
        "counts": lambda: vamp.vamp_det_loss_counts(d, tg.heat, tg.masks, counts, _stream()),
        "forward": lambda: vamp.vamp_det_loss_forward(d, table, tg.heat, tg.anno, tg.inds, tg.masks, counts, loss,
                                                      terms, ws, ws.numel(), _stream()),
        "backward": lambda: vamp.vamp_det_loss_backward(d, table, tg.heat, tg.anno, tg.inds, tg.masks, counts, one,
                                                        gtable, ws, ws.numel(), _stream()),
    }
    fns["counts"]()
    graphs = {k: captured(fn, calls=10) for k, fn in fns.items()}
    res = alternated({k: g.replay for k, g in graphs.items()}, rounds, iters)
    return {f"{k}_us": round(v / 10, 1) for k, v in res.items()}


def step_rows(dev, steps, warm):
    torch.manual_seed(0)
    bb, hd = M.reference_confs(CFG_A)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(CFG_A.sdf_bias)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    data = M.synthetic_batch(CFG_A, 1, seed=0, device=dev, num_points=30000, num_boxes=30)
    fns = {k: M.MultiTaskLoss(model, sdf_bias=CFG_A.sdf_bias, det_targets="device", det_loss=k)
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
    ap.add_argument("--torch-graph", action="store_true",
                    help="afterwards, capture the torch path too and time its replay against the device path's")
    ap.add_argument("--step", action="store_true", help="also time multitask_step at cfg-A with det_loss host / device")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, cases = [], []
    for cname, cfg in (("A", CFG_A), ("B", CFG_B)):
        for B in (1, 8):
            head, tg, preds = make_case(cfg, B, dev)
            leaves = [v for pd in preds for v in pd[0].values()]

            def torch_path(head=head, tg=tg.as_tuple(), preds=preds, leaves=leaves):
                loss = head.loss(tg, [[dict(pd[0])] for pd in preds])
                return torch.autograd.grad(loss, leaves)

            def device_path(head=head, tg=tg, preds=preds, leaves=leaves):
                return torch.autograd.grad(head.loss_device(tg, preds), leaves)

            g_dev = captured(device_path)
            res = alternated({"torch_us": torch_path, "device_us": device_path, "device_graph_us": g_dev.replay},
                             args.rounds, args.iters)
            row = dict(cfg=cname, side=tg.fw, B=B, boxes=40, **res, **kernel_split(head, tg, preds, args.rounds, args.iters))
            rows.append(row)
            cases.append((row, head, tg, preds, leaves, g_dev))
            print(json.dumps(row), flush=True)
    if args.torch_graph:
        # loss uploads its code weights from pageable host memory on every call (new_tensor of a list), which a
        # capture refuses; for the replayed figure the weights are uploaded once and loss runs on a stand-in head
        # that holds them as a device tensor (new_tensor then copies on the device): the same kernels otherwise
        warnings.filterwarnings("ignore", message="To copy construct from a tensor")
        for row, head, tg, preds, leaves, g_dev in cases:
            stub = types.SimpleNamespace(train_cfg=dict(code_weights=torch.tensor(head.train_cfg["code_weights"],
                                                                                  device=dev)),
                                         loss_bbox_weight=head.loss_bbox_weight)
            tgt = tg.as_tuple()

            def torch_path(stub=stub, tgt=tgt, preds=preds, leaves=leaves):
                loss = M.BEVDepthHead.loss(stub, tgt, [[dict(pd[0])] for pd in preds])
                return torch.autograd.grad(loss, leaves)

            try:
                g_torch = captured(torch_path)
            except Exception as e:  # noqa: BLE001
                row["torch_graph"] = f"not capturable: {type(e).__name__}: {str(e).splitlines()[0][:160]}"
                print(json.dumps(row), flush=True)
                continue
            res = alternated({"torch_graph_us": g_torch.replay, "device_graph_again_us": g_dev.replay}, args.rounds,
                             args.iters)
            row.update(res)
            print(json.dumps(row), flush=True)
    if args.step:
        row = dict(step="multitask_step cfg-A B=1", **{f"det_loss_{k}_ms": v for k, v in step_rows(dev, 8, 3).items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
