"""Time the point queries of a step (bv2:576-609) as the module runs them today against the one fused operator.

    python tools/time_point_queries.py [--iters 10] [--rounds 7] [--json profiles/point_queries.json]
                                       [--batches 1,8] [--dtypes float32,bfloat16]

Shapes: cfg-B volumes (K = 18 semantic channels and the density), 34 720 lidar points per sample (one nuScenes
sweep), the 200 x 200 x 16 Occ3D grid rotated by bda.
  split   the four-call sequence of BaseVAMPIRE2._sweep_from_feats: per sample `sample_points(semantic[[i]], border,
          channel_last)` and `sample_points(density[[i]], mask_outside)`, then `occupancy_queries` (2 B + 2 forward
          launches, 2 B + 2 autograd nodes)
  fused   one `HotPath.point_queries` call on per-sample lists, padded inside, as the module hands them over
Modes: batch 1 and 8; fp32 and bf16 volumes (both contenders read the bf16 volumes in place); forward alone and
forward + backward (random upstream gradients through torch.autograd.grad); eager on the current stream.  The two
contenders alternate in one process, `rounds` rounds of `iters` calls each between two device events; a row reports
the median round.  The baseline is `split` in the same run on the same GPU; no ratio is fixed in advance.

Replayed from a graph: NOT MEASURED, and this tool has no such mode.  Its first version captured each contender in a
graph of its own and the first replay ended in a GPU memory-access fault (DESIGN 8.18 has what was seen and what is
only supposed); the mode was taken out with the cause unconfirmed.  The operator's own capture and replay is covered by
tests/test_point_queries.py::test_no_sync_and_graph_replay.

grad_bytes_est is an ESTIMATE of the traffic on the gradient volumes alone, from the shapes (fp32 gradients): with
Vb = C * Z * Y * X * 4 bytes per sample and channel set C in (K, 1),
  split   kernels write (B + B) Vb; every `[[i]]` backward fills a zero [B, ...] tensor and adds one slice
          (B * (B + 2) Vb); autograd adds B + 1 addends of B Vb each, reading two and writing one (3 B^2 Vb)
  fused   B Vb, written once.
Needs the GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import synthetic  # noqa: E402
from vampire_amd.config import CFG_B as cfg  # noqa: E402
from vampire_amd.geometry import make_occ_coords  # noqa: E402
from vampire_amd.ops import HotPath  # noqa: E402

POINTS = 34720


def make_inputs(B, dtype, dev, seed=4):
    dens, sem = (t.to(dev) for t in synthetic.render_inputs(cfg, B, seed=seed)[:2])
    gen = torch.Generator().manual_seed(seed)
    lo = torch.tensor([b[0] for b in (cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg)])
    hi = torch.tensor([b[1] for b in (cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg)])
    pts = ((torch.rand(B, POINTS, 3, generator=gen) * 1.04 - 0.02) * (hi - lo) + lo).to(dev)     # 2 % outside per side
    return dict(sem=sem.to(dtype), dens=dens.to(dtype), pts=pts, bda=synthetic.bda_matrix(B, rot_deg=5.0).to(dev),
                occ=make_occ_coords().to(dev), beta=torch.tensor(0.1, device=dev))


def split(hp, i, s, d, beta):
    outs = []
    for b in range(s.shape[0]):
        p = i["pts"][b][None]
        outs.append(hp.sample_points(s[[b]], p, padding="border", channel_last=True)[0])
        outs.append(hp.sample_points(d[[b]], p, mask_outside=True)[0, 0])
    outs += list(hp.occupancy_queries(s, d, i["occ"], i["bda"], beta))
    return outs


def fused(hp, i, s, d, beta):
    occ_pts = hp.occupancy_points(i["occ"], i["bda"])
    return list(hp.point_queries(s, d, beta, points=list(i["pts"]), sdf=True, occ_points=occ_pts,
                                 lattice=tuple(i["occ"].shape[:3])))


def make_step(hp, i, which, bwd):
    """A callable running one forward (+ backward) on leaves of its own."""
    s, d = i["sem"].clone().requires_grad_(bwd), i["dens"].clone().requires_grad_(bwd)
    beta = i["beta"].clone().requires_grad_(bwd)
    call = (lambda: split(hp, i, s, d, beta)) if which == "split" else (lambda: fused(hp, i, s, d, beta))
    ups = None
    if bwd:
        gen = torch.Generator().manual_seed(1)
        ups = [torch.randn(o.shape, generator=gen).to(o.device) for o in call()]

    def step():
        outs = call()
        if bwd:
            return torch.autograd.grad(outs, [s, d, beta], ups)
        return outs
    return step


def round_us(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def grad_bytes(B, which):
    V = cfg.vZ * cfg.vY * cfg.vX * 4
    tot = 0
    for C in (cfg.num_classes, 1):
        vb = C * V
        tot += B * vb if which == "fused" else (2 * B + B * (B + 2) + 3 * B * B) * vb
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    args = ap.parse_args()
    assert args.rounds >= 7, "the median of at least 7 rounds"
    dev = torch.device("cuda:0")
    hp = HotPath(cfg, dev)
    rows = []
    for B in (int(b) for b in args.batches.split(",")):
        for dtype in (getattr(torch, n) for n in args.dtypes.split(",")):
            i = make_inputs(B, dtype, dev)
            for bwd in (False, True):
                fns = {w: make_step(hp, i, w, bwd) for w in ("split", "fused")}
                for fn in fns.values():
                    fn()
                torch.cuda.synchronize()
                seen = {w: [] for w in fns}
                for _ in range(args.rounds):
                    for w, fn in fns.items():          # the contenders alternate
                        seen[w].append(round_us(fn, args.iters))
                med = {w: statistics.median(v) for w, v in seen.items()}
                row = dict(B=B, volumes=str(dtype).split(".")[-1], mode="eager",
                           passes="forward+backward" if bwd else "forward",
                           split_us=round(med["split"], 1), fused_us=round(med["fused"], 1),
                           split_over_fused=round(med["split"] / med["fused"], 2),
                           split_min_max_us=[round(min(seen["split"]), 1), round(max(seen["split"]), 1)],
                           fused_min_max_us=[round(min(seen["fused"]), 1), round(max(seen["fused"]), 1)],
                           rounds=args.rounds, iters=args.iters,
                           split_grad_bytes_est=grad_bytes(B, "split") if bwd else 0,
                           fused_grad_bytes_est=grad_bytes(B, "fused") if bwd else 0)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del fns
            del i
            torch.cuda.empty_cache()
    rows.append(dict(mode="graph", note="not measured yet: the tool's replayed mode faulted on the GPU and was taken out"))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
