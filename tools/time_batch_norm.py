"""Time the fused batch norm (vampire_amd.norm.BatchNormAct2d over vamp_bn_*: norm [+ residual] [+ ReLU] as one
autograd node, two or three launches per direction) against the torch sequence on the same GPU, on the image
encoder's five activation shapes at six cameras, 256 x 704 (bf16 and fp32) and the BEV trunk's shapes (fp32).

    python tools/time_batch_norm.py [--rounds 7] [--iters 20] [--json profiles/batch_norm.json] [--step]
    python tools/time_batch_norm.py --bytes-only        # the byte table alone (needs no GPU)

Chains: `norm` (the norm alone), `norm_relu`, `norm_res_relu`; directions: `fwd`, `fwd_bwd`.  Variants, alternated
round by round in one process, `iters` back-to-back calls per round between device events (median and minimum over the
rounds, microseconds per call), each in an eager mode and replayed from a captured graph:
  hip        BatchNormAct2d(act, residual)
  torch      F.batch_norm + add + relu and its autograd
  syncbn     nn.SyncBatchNorm + add + relu without a process group (world size 1: torch takes its plain batch_norm
             path there, the synchronised kernels run from two ranks on only)
`bytes` is what each variant's kernels read and write, from the shapes (E elements of s bytes; r = residual, a = ReLU):
  hip   forward  (3 + r) E s         statistics read x; apply reads x [, residual] and writes y
        backward (5 + 2a + r) E s    partial reads dy, x [, y]; apply reads dy, x [, y] and writes dx [, grad_residual]
  torch forward  (3 + 3r + 2a) E s   batch_norm reads x twice and writes; add reads two and writes; relu reads and writes
        backward (5 + 3a) E s        threshold_backward reads two and writes; batch_norm backward reads dy and x twice
                                     and writes dx (the add's backward moves nothing)
and `roofline` the share of the 8 TB/s HBM peak a variant reaches on ITS bytes.  --step adds multitask_step at cfg-A,
batch 1, with norm="BN" and norm="SyncBN".  --ranks N (under torch.distributed.run) times the hip variant with the
gather between N ranks; no test runs it.  Needs the GPU (except --bytes-only)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import norm as N  # noqa: E402

HBM_PEAK = 8.0e12
IMAGE_SHAPES = [(6, 64, 128, 352), (6, 256, 64, 176), (6, 512, 32, 88), (6, 1024, 16, 44), (6, 2048, 8, 22)]
# the BEV ResNet-18 trunk at cfg-A (80 input channels, 128 x 128 cells, base width 160) and the shared conv
BEV_SHAPES = [(1, 160, 64, 64), (1, 320, 32, 32), (1, 640, 16, 16), (1, 64, 128, 128)]
CHAINS = {"norm": (None, False), "norm_relu": ("relu", False), "norm_res_relu": ("relu", True)}


def variant_bytes(shape, dtype, chain):
    act, res = CHAINS[chain]
    a, r = int(act is not None), int(res)
    es = torch.empty((), dtype=dtype).element_size() * shape[0] * shape[1] * shape[2] * shape[3]
    return dict(hip=dict(fwd=(3 + r) * es, bwd=(5 + 2 * a + r) * es),
                torch=dict(fwd=(3 + 3 * r + 2 * a) * es, bwd=(5 + 3 * a) * es))


def byte_table():
    rows = []
    for shapes, dtypes in ((IMAGE_SHAPES, (torch.bfloat16, torch.float32)), (BEV_SHAPES, (torch.float32,))):
        for shape in shapes:
            for dtype in dtypes:
                for chain in CHAINS:
                    rows.append(dict(shape=list(shape), dtype=str(dtype)[6:], chain=chain,
                                     **{k: v for k, v in variant_bytes(shape, dtype, chain).items()}))
    return rows


class TorchChain(nn.Module):
    def __init__(self, channels, act, sync):
        super().__init__()
        self.bn = (nn.SyncBatchNorm if sync else nn.BatchNorm2d)(channels)
        self.act = act

    def forward(self, x, residual=None):
        y = self.bn(x)
        if residual is not None:
            y = y + residual
        return F.relu(y) if self.act == "relu" else y


def make_call(kind, shape, dtype, chain, direction, dev, group=None):
    """A zero-argument callable running one forward (and backward) of the variant on fixed buffers."""
    act, res = CHAINS[chain]
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g).to(dev, dtype).requires_grad_(direction == "fwd_bwd")
    r = torch.randn(shape, generator=g).to(dev, dtype).requires_grad_(direction == "fwd_bwd") if res else None
    dy = torch.randn(shape, generator=g).to(dev, dtype)
    mod = (N.BatchNormAct2d(shape[1], act=act, process_group=group) if kind == "hip"
           else TorchChain(shape[1], act, kind == "syncbn")).to(dev)
    leaves = [x] + ([r] if res else []) + list(mod.parameters())

    def fwd():
        with torch.no_grad():
            return mod(x, r)

    def fwd_bwd():
        return torch.autograd.grad(mod(x, r), leaves, dy)

    return fwd if direction == "fwd" else fwd_bwd


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def time_case(shape, dtype, chain, direction, dev, rounds, iters, kinds=("hip", "torch", "syncbn"), group=None):
    calls = {}
    for kind in kinds:
        eager = make_call(kind, shape, dtype, chain, direction, dev, group)
        calls[f"{kind}_eager"] = eager
        if group is None:
            try:
                calls[f"{kind}_graph"] = graphed(make_call(kind, shape, dtype, chain, direction, dev))
            except Exception as e:  # noqa: BLE001 -- a variant that cannot be captured must not lose the others
                print(f"{kind} {shape} {chain} {direction}: graph not measured: {str(e).splitlines()[0][:120]}",
                      file=sys.stderr)
                torch.cuda.synchronize()
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            times[k].append(timed(fn, iters))
    nbytes = variant_bytes(shape, dtype, chain)
    row = dict(shape=list(shape), dtype=str(dtype)[6:], chain=chain, direction=direction)
    for k, v in times.items():
        v = sorted(v)
        med = v[len(v) // 2]
        b = nbytes["hip" if k.startswith("hip") else "torch"]
        need = b["fwd"] + (b["bwd"] if direction == "fwd_bwd" else 0)
        row[k] = dict(median_us=round(med, 2), min_us=round(v[0], 2), bytes=need,
                      roofline=round(need / (med * 1e-6) / HBM_PEAK, 4))
    return row


def step_rows(dev, steps, warm):
    from vampire_amd import multitask as M
    from vampire_amd.config import CFG_A
    out = {}
    data = M.synthetic_batch(CFG_A, 1, seed=0, device=dev, num_points=30000, num_boxes=30)
    runs = {}
    for kind in ("BN", "SyncBN"):
        torch.manual_seed(0)
        model = M.VAMPIRE2(*M.reference_confs(CFG_A, norm=kind)).to(dev)
        with torch.no_grad():
            model.backbone.density_conv.bias.fill_(CFG_A.sdf_bias)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
        fn = M.MultiTaskLoss(model, sdf_bias=CFG_A.sdf_bias, det_targets="device", det_loss="device")
        runs[kind] = (model, fn, opt)
        for _ in range(warm):
            M.multitask_step(model, fn, data, optimizer=opt)
    times = {k: [] for k in runs}
    for _ in range(steps):
        for k, (model, fn, opt) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            M.multitask_step(model, fn, data, optimizer=opt)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    for k, v in times.items():
        v = sorted(v)
        out[k] = dict(median_ms=round(v[len(v) // 2], 2), min_ms=round(v[0], 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--bytes-only", action="store_true")
    ap.add_argument("--step", action="store_true", help="also time multitask_step at cfg-A with norm BN / SyncBN")
    ap.add_argument("--ranks", type=int, default=0, help="under torch.distributed.run: the hip variant across N ranks")
    args = ap.parse_args()
    if args.bytes_only:
        for row in byte_table():
            print(json.dumps(row))
        return
    assert torch.cuda.is_available(), "timing needs the MI355X"
    group = None
    if args.ranks:
        import torch.distributed as dist
        dist.init_process_group("nccl")
        assert dist.get_world_size() == args.ranks, "start with torch.distributed.run --nproc_per_node=<ranks>"
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", 0)))
        group = dist.group.WORLD
    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    out = dict(device=torch.cuda.get_device_name(dev), chunk=N.BN_CHUNK, rounds=args.rounds, iters=args.iters,
               ranks=args.ranks or 1, rows=rows)

    def dump():
        if args.json and (group is None or torch.distributed.get_rank() == 0):
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)

    for shapes, dtypes in ((IMAGE_SHAPES, (torch.bfloat16, torch.float32)), (BEV_SHAPES, (torch.float32,))):
        for shape in shapes:
            for dtype in dtypes:
                for chain in CHAINS:
                    for direction in ("fwd", "fwd_bwd"):
                        row = time_case(shape, dtype, chain, direction, dev, args.rounds, args.iters,
                                        kinds=("hip",) if group is not None else ("hip", "torch", "syncbn"), group=group)
                        rows.append(row)
                        print(json.dumps(row), flush=True)
                        dump()
    if args.step and group is None:
        out["multitask_step_cfgA_B1"] = step_rows(dev, 8, 3)
        print(json.dumps(out["multitask_step_cfgA_B1"]), flush=True)
        dump()


if __name__ == "__main__":
    main()
