"""Time the parameter update that ends a training step: vampire_amd.optim.ParamUpdate (vamp_param_update_step: clip,
AdamW and EMA in three launches) against the torch sequences, on the tensor list of VAMPIRE2(*reference_confs(CFG_A))
with random gradients.

    python tools/time_param_update.py [--rounds 7] [--iters 30] [--json profiles/param_update.json]
    python tools/time_param_update.py --count-only          # the tensor counts alone (needs no GPU)
    tools/ktail.sh 0.5 8 tools/time_param_update.py --only hip_eager      # per-kernel times of the three launches

Variants, alternated round by round in one process, `iters` back-to-back steps per round between device events
(median and minimum over the rounds, milliseconds per step):
  hip_eager            ParamUpdate.step()
  hip_graph            the same step captured in a CUDA graph, replayed
  torch_*              clip_grad_norm_ + AdamW (default = foreach on the device, or fused=True) followed by the EMA
                       of every floating-point state entry, as the reference's per-tensor loop (`loop`) or with
                       torch._foreach_* (`foreach`, the fair baseline)
  torch_adamw_only     AdamW alone, no clipping and no EMA: what bench.py's multitask step does today
Launches per step come from torch.profiler's kernel list in a run of its own after the timing (null when the profiler
is not available).  `roofline` is the share of the 8 TB/s HBM peak reached on the bytes the update MUST move: 36 B
per parameter element (p, m, v, ema read and written, g read), 12 B per buffer element (x read, ema read and
written) and 4 B per gradient element for the norm pass.  Needs the GPU (except --count-only)."""
import argparse
import copy
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import multitask as M  # noqa: E402
from vampire_amd.config import CFG_A  # noqa: E402

HBM_PEAK = 8.0e12
LR, WD, MAX_NORM, DECAY = 2e-4, 1e-7, 35.0, 0.9990


def build_model():
    torch.manual_seed(0)
    bb, hd = M.reference_confs(CFG_A)
    return M.VAMPIRE2(bb, hd)


def counts(model):
    params = list(model.parameters())
    floats = [v for v in model.state_dict().values() if v.dtype.is_floating_point]
    return dict(param_tensors=len(params), param_elements=sum(p.numel() for p in params),
                params_up_to_4096=sum(p.numel() <= 4096 for p in params),
                params_fp32_contiguous=all(p.dtype == torch.float32 and p.is_contiguous() for p in params),
                float_state_entries=len(floats), float_state_elements=sum(v.numel() for v in floats))


def must_move_bytes(c):
    buffers = c["float_state_elements"] - c["param_elements"]
    return 36 * c["param_elements"] + 12 * buffers + 4 * c["param_elements"]


class TorchUpdate:
    """clip_grad_norm_ + AdamW + the EMA of every floating-point state entry, as torch offers them."""

    def __init__(self, model, fused, foreach_ema, adamw_only=False):
        self.model, self.foreach_ema, self.updates, self.adamw_only = model, foreach_ema, 0, adamw_only
        self.params = list(model.parameters())
        self.opt = torch.optim.AdamW(self.params, lr=LR, weight_decay=WD, **({"fused": True} if fused else {}))
        self.msd = {k: v for k, v in model.state_dict().items() if v.dtype.is_floating_point}
        self.ema = {k: v.detach().clone() for k, v in self.msd.items()}
        self.ema_list, self.model_list = list(self.ema.values()), [v.detach() for v in self.msd.values()]

    @torch.no_grad()
    def step(self):
        if self.adamw_only:
            self.opt.step()
            return
        torch.nn.utils.clip_grad_norm_(self.params, MAX_NORM)
        self.opt.step()
        self.updates += 1
        d = DECAY * (1 - math.exp(-self.updates / 2000))
        if self.foreach_ema:
            torch._foreach_mul_(self.ema_list, d)
            torch._foreach_add_(self.ema_list, self.model_list, alpha=1.0 - d)
        else:
            for k, v in self.ema.items():                       # the reference's loop: two launches per entry
                v *= d
                v += (1.0 - d) * self.msd[k].detach()


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def kernel_launches(fn):
    """Device kernels of one call, from torch.profiler; None when the profiler cannot trace the device here."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as e:  # noqa: BLE001 -- a missing tracer must not lose the timings
        print(f"profiler unavailable: {e!r}", file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", default=None)
    ap.add_argument("--count-only", action="store_true")
    ap.add_argument("--only", default=None, help="time this one variant (under tools/ktail.sh: its kernels alone)")
    args = ap.parse_args()
    proto = build_model()
    c = counts(proto)
    print(json.dumps(c), flush=True)
    if args.count_only:
        return
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from vampire_amd import optim
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    grads = [torch.randn(p.shape, generator=gen).to(dev) for p in proto.parameters()]

    def replica():
        m = copy.deepcopy(proto).to(dev)
        for p, g in zip(m.parameters(), grads):
            p.grad = g.clone()
        return m

    hip = optim.ParamUpdate(replica(), lr=LR, weight_decay=WD, max_norm=MAX_NORM, ema_decay=DECAY)
    hip_g = optim.ParamUpdate(replica(), lr=LR, weight_decay=WD, max_norm=MAX_NORM, ema_decay=DECAY)
    hip_g.step()                                                # uploads the table before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip_g.step()
    variants = {"hip_eager": hip.step, "hip_graph": graph.replay}
    for fused in (False, True):
        for fe in (False, True):
            name = f"torch_{'fused' if fused else 'default'}_adamw_{'foreach' if fe else 'loop'}_ema"
            if args.only in (None, name):
                variants[name] = TorchUpdate(replica(), fused, fe).step
    if args.only in (None, "torch_adamw_only"):
        variants["torch_adamw_only"] = TorchUpdate(replica(), False, True, adamw_only=True).step
    if args.only is not None:
        variants = {args.only: variants[args.only]}
    for fn in variants.values():                                # warm every variant: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.rounds):
        for k, fn in variants.items():
            times[k].append(timed(fn, args.iters))
    need = must_move_bytes(c)
    rows = []
    for k, v in times.items():
        v = sorted(v)
        med, best = v[len(v) // 2], v[0]
        rows.append(dict(variant=k, median_ms=round(med, 4), min_ms=round(best, 4),
                         roofline=round(need / (med * 1e-3) / HBM_PEAK, 4)))

    def dump():
        out = dict(device=torch.cuda.get_device_name(0), counts=c, must_move_bytes=need, chunk=optim.UPDATE_CHUNK,
                   chunks=dict(param=hip.plan.n_param_chunks, buffer=hip.plan.n_buffer_chunks),
                   rounds=args.rounds, iters=args.iters, rows=rows,
                   hip_stats={k: float(v) for k, v in hip.stats.items()})
        if args.json:
            with open(args.json, "w") as f:
                json.dump(out, f, indent=1)

    for row in rows:
        row["launches"] = None
        print(json.dumps(row), flush=True)
    dump()                                                      # the timings are safe before the profiler starts
    if args.only is not None:
        return
    for row in rows:
        if row["variant"] != "hip_graph":                       # (a replay runs hip_eager's kernels)
            row["launches"] = kernel_launches(variants[row["variant"]])
        print(json.dumps({"variant": row["variant"], "launches": row["launches"]}), flush=True)
    dump()


if __name__ == "__main__":
    main()
