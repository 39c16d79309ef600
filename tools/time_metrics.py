"""Time the segmentation-metric updates (vampire_amd.metrics) against the reference's formulation in torch.

    python tools/time_metrics.py [--iters 200] [--json out.json]

At cfg-B (Occ3D grid 200 x 200 x 16, 18 classes, ~35 000 lidar points per sample) for B = 1 and B = 8:
  occ update     JaccardIndex.update on the backbone's permuted occ_logits view under mask_camera
  occ torch      the reference: occ_logits[mask_camera].argmax(1), bincount(t * Kc + p)
  update_val     SegEvaluator.update_val (lidar-seg prediction + both confusion updates)
  val torch      the reference's validation_step metric code (zeros + index_add_, argmax, bincount, boolean index)
Eager: device events around `iters` back-to-back calls (includes the host's launch cost).  Graph: the same
call captured once in a CUDA graph and replayed (device time of the kernels and the gaps between them).
GB/s of the occupancy update = (logits + targets + mask bytes) / graph time.  Needs the GPU.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import metrics  # noqa: E402

K = 18
GRID = (200, 200, 16)


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
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(10):
            fn()
    return timed(g.replay, max(iters // 10, 5), warmup=2) / 10


def torch_confusion(cm, x, t, Kc):
    cm += torch.bincount(t * Kc + x, minlength=Kc * Kc).reshape(Kc, Kc)


def make_inputs(B, P, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    occ = torch.randn((B, K) + GRID, generator=g).to(dev).permute(0, 2, 3, 4, 1)   # backbone.py:504 view
    sem = torch.randint(0, K, (B,) + GRID, generator=g).to(dev)
    mask = (torch.rand((B,) + GRID, generator=g) < 0.5).to(dev)
    pts = [torch.randn(P, K, generator=g).to(dev) for _ in range(B)]
    nref = P + P // 10
    ref_index = [torch.randint(0, nref, (P,), generator=g).to(dev) for _ in range(B)]
    ref_labels = [torch.randint(0, K - 1, (nref,), generator=g).to(dev) for _ in range(B)]
    batch = [None] * 8 + [ref_labels, ref_index, None, sem, None, None, mask]
    return (pts, occ, None), batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--points", type=int, default=35000)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_metrics needs the GPU"
    dev = torch.device("cuda:0")
    rows = []
    for B in (1, 8):
        outputs, batch = make_inputs(B, a.points, dev)
        occ, sem, mask = outputs[1], batch[11], batch[14]
        j = metrics.JaccardIndex(K, device=dev)
        ev = metrics.SegEvaluator(device=dev)
        cm = torch.zeros(K, K, dtype=torch.int64, device=dev)
        cml = torch.zeros(K - 1, K - 1, dtype=torch.int64, device=dev)

        def occ_ours():
            j.update(occ, sem, mask)

        def occ_torch():
            torch_confusion(cm, occ[mask].argmax(1), sem[mask], K)

        def val_ours():
            ev.update_val(outputs, batch)

        def val_torch():
            for logits, idx, lab in zip(outputs[0], batch[9], batch[8]):
                ref = torch.zeros((len(lab), K), device=dev)
                ref.index_add_(0, idx, logits)
                seg = ref[..., 1:-1].argmax(1) + 1
                keep = lab != 0
                torch_confusion(cml, seg[keep], lab[keep], K - 1)
            occ_torch()

        # the two formulations count the same occupancy matrix
        j.reset()
        cm.zero_()
        occ_ours()
        occ_torch()
        torch.cuda.synchronize()
        assert torch.equal(j.confmat, cm), "occupancy confusion matrices differ"

        nbytes = occ.numel() * 4 + sem.numel() * 8 + mask.numel()
        r = dict(B=B, points=a.points,
                 occ_update_us=timed(occ_ours, a.iters), occ_update_graph_us=timed_graph(occ_ours, a.iters),
                 occ_torch_us=timed(occ_torch, a.iters),
                 update_val_us=timed(val_ours, a.iters), update_val_graph_us=timed_graph(val_ours, a.iters),
                 val_torch_us=timed(val_torch, a.iters), occ_bytes=nbytes)
        r["occ_update_GBps"] = nbytes / (r["occ_update_graph_us"] * 1e-6) / 1e9
        rows.append(r)
        print(f"B={B}: occ update {r['occ_update_us']:.1f} us eager, {r['occ_update_graph_us']:.1f} us graph "
              f"({r['occ_update_GBps']:.0f} GB/s of {nbytes / 1e6:.1f} MB) | torch reference {r['occ_torch_us']:.1f} us"
              f" || update_val {r['update_val_us']:.1f} us eager, {r['update_val_graph_us']:.1f} us graph"
              f" | torch reference {r['val_torch_us']:.1f} us", flush=True)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), rows=rows)))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
