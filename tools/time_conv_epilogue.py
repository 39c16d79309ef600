#!/usr/bin/env python3
"""What `SWITCHES.conv3d_epilogue` buys: act(conv(x, w) + bias + residual) as one kernel and one autograd
node against the unfused path of the same checkout (the switch off), in one process, the two alternating round by
round.  Cases: each layer form of the UNet at its cfg-B volume (16x200x200, 8x100x100, 4x50x50), the three heads at
16x200x200, the whole Unet3D(16, 16), and the whole BaseVAMPIRE2 module as tools/time_backbone.py runs it; forward and
forward + backward, in fp32 and under a bf16 autocast, eager (wall time of the enqueue-and-wait, the host's launches
included) and replayed from a captured graph (device time).  Every shape is warmed first; a figure is the median of the
rounds' means, the spread their min .. max.  Every case is written, wins and losses alike; a mode that could not be run
is written as "not measured" with the reason.
usage: tools/time_conv_epilogue.py [--rounds R] [--reps N] [--out FILE] [--no-module] [--no-module-graph]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vampire_amd import backbone, synthetic                          # noqa: E402
from vampire_amd.config import PRESETS                              # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "conv_epilogue.json"))
ap.add_argument("--no-module", action="store_true")
ap.add_argument("--no-module-graph", action="store_true", help="do not capture the whole module in a graph")
args = ap.parse_args()
assert args.rounds >= 7, "the protocol asks for the median of at least 7 rounds"
assert torch.cuda.is_available(), "this tool times kernels on the GPU"
dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True              # MIOpen find: what a training script sets (backbone.py's note)
SW = backbone.SWITCHES
ROWS = []


def wall_us(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def device_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def contest(fns, timer, reps):
    """{name: (median, min, max)}: the contenders alternate inside every round."""
    t = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            t[k].append(timer(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def capture(step):
    """`step` warmed on a side stream (its workspaces allocated there), then captured on that stream."""
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for _ in range(3):
            step()
    torch.cuda.current_stream(dev).wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        step()
    return graph.replay


def record(case, precision, what, mode, res=None, why=None):
    row = dict(case=case, precision=precision, what=what, mode=mode)
    if res is None:
        row["result"] = "not measured: " + why
        print("%-40s %-5s %-8s %-6s not measured: %s" % (case, precision, what, mode, why), flush=True)
    else:
        off, on = res["off"], res["on"]
        row.update(off_us=[round(v, 1) for v in off], on_us=[round(v, 1) for v in on], on_over_off=round(on[0] / off[0], 3))
        print("%-40s %-5s %-8s %-6s off %9.1f us (%.1f .. %.1f)   on %9.1f us (%.1f .. %.1f)   on/off %.3f" % (
            case, precision, what, mode, *off, *on, on[0] / off[0]), flush=True)
    ROWS.append(row)


def measure(case, make_step, reps, graph=True):
    """make_step(bwd) -> a step function that reads SW.conv3d_epilogue when it runs (eager) or is captured (graph)."""
    for precision, dt16 in (("fp32", None), ("bf16", torch.bfloat16)):
        for what, bwd in (("fwd", False), ("fwd+bwd", True)):
            inner = make_step(bwd)

            def stepper(on):
                def step():
                    SW.conv3d_epilogue = on
                    with torch.autocast("cuda", dtype=dt16, enabled=dt16 is not None):
                        inner()
                return step

            steps = {"off": stepper(False), "on": stepper(True)}
            for fn in steps.values():                       # warm every shape: MIOpen's find, the workspaces
                for _ in range(3):
                    fn()
            record(case, precision, what, "eager", contest(steps, wall_us, reps))
            if not graph:
                record(case, precision, what, "graph", why="skipped on the command line (--no-module-graph)")
                continue
            try:
                replays = {k: capture(fn) for k, fn in steps.items()}
                record(case, precision, what, "graph", contest(replays, device_us, reps))
            except Exception as e:                          # noqa: BLE001 -- a case that cannot be captured is reported
                torch.cuda.synchronize()
                record(case, precision, what, "graph", why="capture failed: " + str(e).splitlines()[0][:120])
    SW.conv3d_epilogue = False


def layer_case(name, cin, cout, stride, vol, residual, leaky):
    torch.manual_seed(0)
    layer = backbone._conv3(cin, cout, stride).to(dev)
    ovol = [(n - 1) // stride + 1 for n in vol]
    x = torch.randn(1, cin, *vol, device=dev, requires_grad=True)
    r = torch.randn(1, cout, *ovol, device=dev, requires_grad=True) if residual else None
    up = torch.randn(1, cout, *ovol, device=dev)

    def make_step(bwd):
        def step():
            # (under autocast the residual arrives in 16 bits from the layer before it)
            rr = None if r is None else (r.to(torch.get_autocast_dtype("cuda")) if torch.is_autocast_enabled() else r)
            with torch.set_grad_enabled(bwd):
                y = backbone._conv3_then(layer, x, rr, leaky)
            if bwd:
                torch.autograd.grad(y, [x, layer.weight] + ([r] if r is not None else []), up.to(y.dtype))
        return step

    measure("%s %d->%d s%d %s" % (name, cin, cout, stride, "x".join(map(str, vol))), make_step, args.reps)


class Heads(torch.nn.Module):
    """The backbone's three heads over the same three layers (`BaseVAMPIRE2._heads`)."""

    def __init__(self, mid, num_classes):
        super().__init__()
        self.num_classes = num_classes
        self.density_conv = torch.nn.Conv3d(mid, 1, 3, 1, 1, bias=True)
        self.seg_conv = torch.nn.Conv3d(mid, num_classes, 3, 1, 1, bias=True)
        self.rgb_conv = torch.nn.Sequential(torch.nn.Conv3d(mid, 3, 3, 1, 1, bias=True), torch.nn.Sigmoid())

    def forward(self, base):
        return backbone.BaseVAMPIRE2._heads(self, base)


def net_case(name, net, x, reps):
    params = [p for p in net.parameters()]

    def make_step(bwd):
        def step():
            with torch.set_grad_enabled(bwd):
                outs = net(x)
            if bwd:
                outs = outs if isinstance(outs, tuple) else (outs,)
                torch.autograd.grad(sum(o.float().mean() for o in outs), [x] + params, allow_unused=True)
        return step

    measure(name, make_step, reps)


def module_case():
    c = PRESETS["B"]
    kw = dict(x_bound_seg=list(c.x_bound_seg), y_bound_seg=list(c.y_bound_seg), z_bound_seg=list(c.z_bound_seg),
              x_bound_det=list(c.x_bound_det), y_bound_det=list(c.y_bound_det), z_bound_det=list(c.z_bound_det),
              d_bound=list(c.d_bound), final_dim=c.final_dim, downsample_factor=4, upsample_factor=4,
              mid_channels=c.mid_channels, output_channels=80, img_backbone_conf=dict(),
              img_neck_conf=dict(out_channels=[128] * 4), num_classes=c.num_classes, density_mode="sdf",
              sdf_bias=-1.0, cat_pos=False, cat_seg=False)
    torch.manual_seed(0)
    mod = backbone.BaseVAMPIRE2(**kw).to(dev)
    s2e, K, ida = synthetic.camera_rig(c, 1, seed=0)
    mats = {k: v.to(dev) for k, v in dict(sensor2ego_mats=s2e[:, None], intrin_mats=K[:, None], ida_mats=ida[:, None],
                                          sensor2sensor_mats=torch.eye(4).expand(1, 1, 6, 4, 4).contiguous(),
                                          bda_mat=synthetic.bda_matrix(1)).items()}
    imgs = torch.randn(1, 1, 6, 3, *c.final_dim, device=dev)

    def make_step(bwd):
        def step():
            mod.zero_grad(set_to_none=True)
            with torch.set_grad_enabled(bwd):
                out = mod(imgs, mats)
            if bwd:
                sum(o.float().mean() for o in out if torch.is_tensor(o) and o.requires_grad).backward()
        return step

    measure("BaseVAMPIRE2 cfg-B batch 1", make_step, 3, graph=not args.no_module_graph)


print("rounds %d; median of the rounds' means (min .. max); eager = wall time, graph = device time of a replay" % args.rounds)
layer_case("conv1 +leaky", 16, 32, 2, (16, 200, 200), False, True)
layer_case("conv2 +res+leaky", 32, 32, 1, (8, 100, 100), True, True)
layer_case("conv3 +leaky", 32, 32, 2, (8, 100, 100), False, True)
layer_case("conv4 +leaky", 32, 32, 1, (4, 50, 50), False, True)
layer_case("conv5 +res+leaky", 32, 32, 1, (8, 100, 100), True, True)
layer_case("conv6 +res", 32, 16, 1, (16, 200, 200), True, False)
torch.manual_seed(0)
net_case("heads 16->1+18+3 16x200x200", Heads(16, 18).to(dev),
         torch.randn(1, 16, 16, 200, 200, device=dev, requires_grad=True), args.reps)
torch.manual_seed(0)
net_case("Unet3D(16,16) 16x200x200", backbone.Unet3D(16, 16).to(dev),
         torch.randn(1, 16, 16, 200, 200, device=dev, requires_grad=True), 5)


def dump():
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), rounds=args.rounds,
                       protocol="switch off and on alternate inside every round; median of the rounds' means [median, min, "
                                "max] in microseconds; eager = wall time per step, graph = device time per replay",
                       rows=ROWS), f, indent=1)
        f.write("\n")


dump()                                  # (the module is the one case whose capture may not succeed: keep the rest)
if not args.no_module:
    module_case()
    dump()
print("wrote", args.out)
