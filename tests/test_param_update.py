"""The device parameter update (vampire_amd.optim.ParamUpdate over vamp_param_update_step) against torch's own
clip_grad_norm_ + AdamW(foreach=False) + the reference's EMA loop in float64 on the CPU.

Bar, per tensor: err = max|x - x64| / max|x64|.  The HIP path may reach max(2 E_torch, 2^-22), E_torch being the same
error of the fp32 torch sequence on the same GPU and 2^-22 the final fp32 rounding plus at most three intermediate
roundings of quantities at the result's scale.  total_norm is within one fp32 ulp of sqrt(math.fsum(g g)).  All
tensors are tiny (sizes around the chunk edges, about 25 k elements in all)."""
import copy
import functools
import math

import numpy as np
import pytest
import torch

from vampire_amd import optim

pytestmark = pytest.mark.gpu

CH = optim.UPDATE_CHUNK
EDGE_SIZES = [1, 3, CH - 1, CH, CH + 1, 2 * CH + 3]
FLOOR = 2.0 ** -22
BETAS, EPS, DECAY, UPDATES0 = (0.9, 0.999), 1e-8, 0.9990, 1000


class Net(torch.nn.Module):
    """Conv-BN-Linear, a multi-chunk buffer, and parameters at the chunk edges (registered last: the table's last
    parameter chunk is the 3-element tail of the 2 CH + 3 tensor)."""

    def __init__(self, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.conv = torch.nn.Conv2d(3, 5, 3, bias=False)       # (a bias in front of a BatchNorm has no gradient)
        self.bn = torch.nn.BatchNorm2d(5)
        self.lin = torch.nn.Linear(5, 3)
        self.register_buffer("table", torch.randn(CH + 5, generator=gen))
        self.edges = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=gen)) for n in EDGE_SIZES])
        with torch.no_grad():
            for p in list(self.conv.parameters()) + list(self.bn.parameters()) + list(self.lin.parameters()):
                p.copy_(torch.randn(p.shape, generator=gen))
            self.bn.running_mean.copy_(torch.randn(5, generator=gen))
            self.bn.running_var.copy_(torch.rand(5, generator=gen) + 0.5)
            self.bn.num_batches_tracked.fill_(7)

    def forward(self, x, _unused=None, inrange_pts=None, lidar_seg=False):
        return self.lin(self.bn(self.conv(x)).mean(dim=(2, 3)))


def float_buffers(model):
    params = {id(p) for p in model.parameters()}
    return [(k, v) for k, v in model.state_dict(keep_vars=True).items()
            if v.dtype.is_floating_point and id(v) not in params]


def make_case(norm, weight_decay, steps=5, seed=1, bad=None, scales=None, lrs=None, max_norm=35.0, wide=False):
    """Everything a run needs, as fp32 CPU tensors shared by the three runs: initial values, one gradient set and one
    set of buffer values per step (the gradients already multiplied by the scale they carry)."""
    gen = torch.Generator().manual_seed(seed)
    net = Net(seed)
    shapes = [p.shape for p in net.parameters()]
    total = sum(math.prod(s) for s in shapes)
    scales, bad = list(scales or [1.0] * steps), dict(bad or {})
    grads = []
    for k in range(steps):
        if wide:                                      # magnitudes 2^-20 .. 2^20: power-of-two scaling stays exact
            gs = [torch.exp2(torch.rand(s, generator=gen) * 40 - 20) * (torch.randint(0, 2, s, generator=gen) * 2 - 1)
                  for s in shapes]
        else:
            gs = [torch.randn(s, generator=gen) * (norm / math.sqrt(total)) for s in shapes]
        grads.append([(g * scales[k]).float() for g in gs])
    for k, where in bad.items():
        if where == "inf-first":
            grads[k][0].view(-1)[0] = float("inf")
        else:
            grads[k][-1].view(-1)[-1] = float("nan")
    bufs = [[torch.randn(v.shape, generator=gen) for _, v in float_buffers(net)] for _ in range(steps)]
    return dict(net=net, grads=grads, bufs=bufs, scales=scales, lrs=list(lrs or [1e-3] * 3 + [5e-4] * (steps - 3)),
                skip=[k in bad for k in range(steps)], weight_decay=weight_decay, max_norm=max_norm, steps=steps)


def ema_loop(ema_sd, model_sd, updates, decay):
    """The reference's averaged-weights update, restated: every floating-point state entry, two in-place ops."""
    d = decay * (1 - math.exp(-updates / 2000))
    for k, v in ema_sd.items():
        if v.dtype.is_floating_point:
            v *= d
            v += (1.0 - d) * model_sd[k].detach()


def run_torch(case, dtype, device):
    """clip_grad_norm_ + AdamW(foreach=False) + the EMA loop in `dtype` on `device`; a skipped step moves the EMA only.
    `case["net"]` is any module (tests/test_step_kernels_sweep.py brings its own); `case["betas"]` stands in for BETAS."""
    net = copy.deepcopy(case["net"]).to(device=device, dtype=dtype)
    if hasattr(net, "bn"):
        net.bn.num_batches_tracked.fill_(7)
    ema = {k: v.detach().clone() for k, v in net.state_dict().items()}
    params = list(net.parameters())
    opt = torch.optim.AdamW(params, lr=case["lrs"][0], betas=case.get("betas", BETAS), eps=EPS,
                            weight_decay=case["weight_decay"], foreach=False)
    updates = UPDATES0
    for k in range(case["steps"]):
        with torch.no_grad():
            for (_, b), val in zip(float_buffers(net), case["bufs"][k]):
                b.copy_(val)
        for g in opt.param_groups:
            g["lr"] = case["lrs"][k]
        if not case["skip"][k]:
            for p, g in zip(params, case["grads"][k]):
                p.grad = g.to(device=device, dtype=dtype) / case["scales"][k]
            if case["max_norm"] > 0:
                torch.nn.utils.clip_grad_norm_(params, case["max_norm"], foreach=False)
            opt.step()
        updates += 1
        with torch.no_grad():
            ema_loop(ema, net.state_dict(), updates, DECAY)
    out = {"p": [p.detach() for p in params],
           "m": [opt.state[p]["exp_avg"] for p in params], "v": [opt.state[p]["exp_avg_sq"] for p in params],
           "ema": [ema[k] for k, v in ema.items() if v.dtype.is_floating_point]}
    return {name: [t.double().cpu() for t in ts] for name, ts in out.items()}


def hip_state(net, upd):
    """p, m, v and the EMA of every float entry, as fp32 CPU tensors in run_torch's order."""
    pl = upd.plan
    params = list(net.parameters())
    offs = pl.tensor_state_offset.tolist()
    m = [upd.exp_avg[o:o + p.numel()].view(p.shape) for p, o in zip(params, offs)]
    v = [upd.exp_avg_sq[o:o + p.numel()].view(p.shape) for p, o in zip(params, offs)]
    ema = [t for t in upd.ema_state_dict().values() if t.dtype.is_floating_point]
    out = {"p": [p.detach() for p in params], "m": m, "v": v, "ema": ema}
    return {name: [t.detach().cpu().clone() for t in ts] for name, ts in out.items()}


def run_hip(case, loss_scale=None, dev="cuda", observe=None):
    net = copy.deepcopy(case["net"]).to(dev)
    upd = optim.ParamUpdate(net, lr=case["lrs"][0], betas=BETAS, eps=EPS, weight_decay=case["weight_decay"],
                            max_norm=case["max_norm"], ema_decay=DECAY, ema_updates=UPDATES0, loss_scale=loss_scale)
    params = list(net.parameters())
    stats = []
    for k in range(case["steps"]):
        with torch.no_grad():
            for (_, b), val in zip(float_buffers(net), case["bufs"][k]):
                b.copy_(val)
        if k > 0 and case["lrs"][k] != case["lrs"][k - 1]:
            upd.set_lr(case["lrs"][k])
        for p, g in zip(params, case["grads"][k]):
            p.grad = g.to(dev)
        before = hip_state(net, upd) if observe == k else None
        upd.step()
        stats.append({key: val.item() for key, val in upd.stats.items()})
        if observe == k:
            stats[-1]["before"], stats[-1]["after"] = before, hip_state(net, upd)
    return hip_state(net, upd), stats


@functools.lru_cache(maxsize=None)
def oracle(key):
    """The case and its float64 CPU result, computed once per configuration and never modified."""
    case = make_case(**dict(key))
    return case, run_torch(case, torch.float64, "cpu")


def rel_err(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max())


def check_against_oracle(case, ref, got, label):
    e_torch = run_torch(case, torch.float32, "cuda")
    worst = 0.0
    for name in ("p", "m", "v", "ema"):
        assert len(got[name]) == len(ref[name])
        for i, (x, t, r) in enumerate(zip(got[name], e_torch[name], ref[name])):
            e_hip, e_t = rel_err(x, r), rel_err(t, r)
            print(f"{label} {name}[{i}] n={r.numel()}: hip {e_hip:.3e}  torch fp32 {e_t:.3e}")
            assert e_hip <= max(2 * e_t, FLOOR), (label, name, i, e_hip, e_t)
            worst = max(worst, e_hip)
    return worst


def norm_reference(grads, scale):
    return math.sqrt(math.fsum(float(x) ** 2 for g in grads for x in (g.double() / scale).view(-1).tolist()))


def assert_within_one_ulp(value, ref):
    assert abs(value - ref) <= float(np.spacing(np.float32(ref))), (value, ref)


# ----------------------------------------------------------------------------------------------- 1. five steps
@pytest.mark.parametrize("weight_decay", [0.01, 0.0])
@pytest.mark.parametrize("norm", [100.0, 1.0])
def test_five_steps_match_the_float64_oracle(norm, weight_decay):
    case, ref = oracle((("norm", norm), ("weight_decay", weight_decay)))
    got, stats = run_hip(case)
    for k, st in enumerate(stats):
        assert st["found_inf"] == 0 and st["step"] == k + 1 and st["updates"] == UPDATES0 + k + 1 and st["scale"] == 1.0
        tn = norm_reference(case["grads"][k], 1.0)
        print(f"step {k}: total_norm {st['total_norm']!r} reference {tn!r} clip_coef {st['clip_coef']!r}")
        assert_within_one_ulp(st["total_norm"], tn)
        if norm == 1.0:
            assert st["clip_coef"] == 1.0                       # exactly: the gradients pass unchanged
        else:
            assert 0.3 < st["clip_coef"] < 0.4
            assert_within_one_ulp(st["clip_coef"], 35.0 / (tn + 1e-6))
    check_against_oracle(case, ref, got, f"norm={norm} wd={weight_decay}")


# ----------------------------------------------------------------------------------------------- 2. overflow
@pytest.mark.parametrize("where", ["inf-first", "nan-last"])
def test_overflow_skips_the_step_and_halves_the_scale(where):
    scales = (65536.0, 65536.0, 32768.0)
    case, ref = oracle((("norm", 100.0), ("weight_decay", 0.01), ("steps", 3), ("bad", ((1, where),)),
                        ("scales", scales), ("lrs", (1e-3,) * 3)))
    got, stats = run_hip(case, loss_scale="dynamic", observe=1)
    assert [s["found_inf"] for s in stats] == [0, 1, 0]
    assert [s["step"] for s in stats] == [1, 1, 2]              # t did not advance on the bad step
    assert [s["updates"] for s in stats] == [UPDATES0 + 1, UPDATES0 + 2, UPDATES0 + 3]
    assert [s["scale"] for s in stats] == [65536.0, 32768.0, 32768.0]
    assert not math.isfinite(stats[1]["total_norm"])
    before, after = stats[1]["before"], stats[1]["after"]
    for name in ("p", "m", "v"):
        for a, b in zip(before[name], after[name]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name      # bit for bit
    moved = [not torch.equal(a, b) for a, b in zip(before["ema"], after["ema"])]
    assert all(moved), moved                                    # the EMA ran on the unchanged weights
    assert_within_one_ulp(stats[2]["total_norm"], norm_reference(case["grads"][2], 32768.0))
    check_against_oracle(case, ref, got, where)                 # the clean step after it: an oracle that skipped


# ----------------------------------------------------------------------------------------------- 3. scaled gradients
def test_power_of_two_loss_scale_is_bitwise_invisible():
    """Power-of-two scaling is exact in fp32 and float64 at these magnitudes, so the two runs must agree bit for bit."""
    plain = make_case(0.0, 0.01, steps=3, wide=True, lrs=[1e-3] * 3)
    scaled = dict(plain, grads=[[g * 1024.0 for g in gs] for gs in plain["grads"]])
    for gs in scaled["grads"]:
        assert all(torch.isfinite(g).all() for g in gs)
    a, sa = run_hip(plain)
    b, sb = run_hip(scaled, loss_scale=1024.0)
    for x, y in zip(sa, sb):
        assert x["total_norm"] == y["total_norm"] and x["clip_coef"] == y["clip_coef"] and x["clip_coef"] < 1.0
        assert (x["scale"], y["scale"]) == (1.0, 1024.0) and x["found_inf"] == y["found_inf"] == 0
    for name in ("p", "m", "v", "ema"):
        for x, y in zip(a[name], b[name]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


# ----------------------------------------------------------------------------------------------- 4. placement
class Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def run_bag(values, grads, steps=2, **kw):
    """`values`, `grads`: device tensors used as they are (their addresses are the point)."""
    bag = Bag(values)
    assert all(p.data_ptr() == t.data_ptr() for p, t in zip(bag.ps, values))
    upd = optim.ParamUpdate(bag, lr=1e-2, weight_decay=0.01, ema_updates=UPDATES0, **kw)
    for _ in range(steps):
        for p, g in zip(bag.ps, grads):
            p.grad = g
        upd.step()
    offs = upd.plan.tensor_state_offset.tolist()
    out = []
    for p, o in zip(bag.ps, offs):
        n = p.numel()
        out.append(tuple(t.detach().cpu().clone().view(torch.int32)
                         for t in (p, upd.exp_avg[o:o + n], upd.exp_avg_sq[o:o + n], upd.ema[o:o + n])))
    return out


@pytest.fixture(scope="module")
def placement_data():
    gen = torch.Generator().manual_seed(5)
    n = CH + 5                                    # a full chunk of 16-byte groups and a tail that crosses the end
    x, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    base = run_bag([x.cuda()], [g.cuda()])[0]
    return n, x, g, base


@pytest.mark.parametrize("p_off,g_off", [(1, 1), (2, 2), (3, 3), (1, 0), (0, 2)])
def test_a_slice_at_any_offset_gives_the_bits_of_an_aligned_copy(placement_data, p_off, g_off):
    n, x, g, base = placement_data
    big_x, big_g = torch.zeros(n + 8, device="cuda"), torch.zeros(n + 8, device="cuda")
    big_x[p_off:p_off + n] = x.cuda()
    big_g[g_off:g_off + n] = g.cuda()
    xs, gs = big_x[p_off:p_off + n], big_g[g_off:g_off + n]
    assert xs.data_ptr() % 16 == 4 * p_off and gs.data_ptr() % 16 == 4 * g_off
    got = run_bag([xs], [gs])[0]
    for a, b in zip(got, base):
        assert torch.equal(a, b)
    assert float(big_x[:p_off].abs().sum()) == 0 and float(big_x[p_off + n:].abs().sum()) == 0   # nothing outside it


def test_a_tensor_does_not_depend_on_the_tensors_in_front_of_it(placement_data):
    """Without clipping (the norm couples the tensors) a tensor's p, m, v and EMA are its own."""
    n, x, g, _ = placement_data
    gen = torch.Generator().manual_seed(6)
    alone = run_bag([x.cuda()], [g.cuda()], max_norm=0.0)[0]
    junk = [torch.randn(k, generator=gen).cuda() for k in (3, CH + 1, 70)]
    junk_g = [torch.randn(k, generator=gen).cuda() for k in (3, CH + 1, 70)]
    behind = run_bag(junk + [x.cuda()], junk_g + [g.cuda()], max_norm=0.0)[-1]
    for a, b in zip(alone, behind):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------- 5. repeatability
def test_two_identical_runs_are_bitwise_equal():
    case, _ = oracle((("norm", 100.0), ("weight_decay", 0.01)))
    a, sa = run_hip(case)
    b, sb = run_hip(case)
    assert sa == sb
    for name in ("p", "m", "v", "ema"):
        for x, y in zip(a[name], b[name]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


# ----------------------------------------------------------------------------------------------- 6. no host sync
def test_step_does_not_synchronise_the_host():
    net = Net(2).cuda()
    upd = optim.ParamUpdate(net, lr=1e-3, ema_updates=UPDATES0, loss_scale="dynamic")
    params = list(net.parameters())
    first = [torch.randn_like(p) for p in params]
    second = [torch.randn_like(p) for p in params]
    loss = torch.ones((), device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for grads in (first, first, second):                    # an upload, the same addresses, another upload
            for p, g in zip(params, grads):
                p.grad = g
            upd.step()
            upd.set_lr(5e-4)
            scaled = upd.scale_loss(loss)
        upd.zero_grad(set_to_none=False)
        upd.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert upd.stats["step"].item() == 4 and float(scaled) == 65536.0


# ----------------------------------------------------------------------------------------------- 7. graph replay
def test_a_captured_step_replays_like_eager_steps():
    gen = torch.Generator().manual_seed(9)
    proto = Net(3)
    gsets = [[torch.randn(p.shape, generator=gen) for p in proto.parameters()] for _ in range(4)]

    def prepare():
        net = copy.deepcopy(proto).cuda()
        upd = optim.ParamUpdate(net, lr=1e-3, weight_decay=0.01, ema_updates=UPDATES0, loss_scale="dynamic")
        params = list(net.parameters())
        for p, g in zip(params, gsets[0]):
            p.grad = (g * 65536.0).cuda()
        upd.step()                                              # eager: uploads the table of these gradient tensors
        return net, upd, params

    def load(params, k):
        with torch.no_grad():
            for p, g in zip(params, gsets[k]):
                p.grad.copy_((g * 65536.0).cuda())              # in place: the addresses stay

    stream = torch.cuda.Stream()
    results = []
    with torch.cuda.stream(stream):                             # every tensor is made on the capture stream
        for replay in (False, True):
            net, upd, params = prepare()
            graph = None
            if replay:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=stream):
                    upd.step()
            for k in (1, 2, 3):
                load(params, k)
                graph.replay() if replay else upd.step()
            stream.synchronize()
            results.append((hip_state(net, upd), {key: val.item() for key, val in upd.stats.items()}))
        # a gradient that moved: refused while capturing, before anything is launched
        spare = torch.zeros_like(params[0])
        marker = torch.zeros(4, device="cuda")
        steps_before = upd.stats["step"].item()
        refused = torch.cuda.CUDAGraph()
        with torch.cuda.graph(refused, stream=stream):
            marker.add_(1.0)
            params[0].grad = spare
            with pytest.raises(RuntimeError, match="set_to_none=False"):
                upd.step()
        refused.replay()
        stream.synchronize()
        assert upd.stats["step"].item() == steps_before and float(marker[0]) == 1.0
    (eager, es), (replayed, rs) = results
    assert es == rs and es["step"] == 4 and es["updates"] == UPDATES0 + 4 and es["found_inf"] == 0
    for name in ("p", "m", "v", "ema"):
        for x, y in zip(eager[name], replayed[name]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), name


# ----------------------------------------------------------------------------------------------- 8. EMA access
def test_ema_state_dict_copy_and_the_multitask_step_calls():
    from vampire_amd.multitask import multitask_step
    net = Net(4).cuda()
    upd = optim.ParamUpdate(net, lr=1e-2, ema_updates=UPDATES0)
    before = [p.detach().clone() for p in net.parameters()]
    x = torch.randn(2, 3, 6, 6, device="cuda")
    batch = [x] + [None] * 11
    for _ in range(2):
        loss = multitask_step(net, lambda out, b: out.square().mean(), batch, optimizer=upd, amp_dtype=None)
    assert torch.isfinite(loss) and upd.stats["step"].item() == 2 and upd.stats["found_inf"].item() == 0
    used = list(net.conv.parameters()) + list(net.bn.parameters()) + list(net.lin.parameters())
    assert all(p.grad is not None for p in used) and all(p.grad is None for p in net.edges)
    for p, b in zip(net.parameters(), before):
        changed = not torch.equal(p.detach(), b)
        assert changed == any(p is q for q in used)             # a parameter without a gradient is skipped
    sd, esd = net.state_dict(), upd.ema_state_dict()
    assert list(esd.keys()) == list(sd.keys())
    assert int(sd["bn.num_batches_tracked"]) == 9 and int(esd["bn.num_batches_tracked"]) == 7
    for k, v in esd.items():
        assert v.shape == sd[k].shape and v.dtype == sd[k].dtype
        if v.dtype.is_floating_point:
            assert v.data_ptr() >= upd.ema.data_ptr() and v.data_ptr() < upd.ema.data_ptr() + 4 * upd.ema.numel()
    assert not torch.equal(esd["bn.running_mean"], sd["bn.running_mean"])    # the buffers' EMA lags the buffers
    assert not torch.equal(esd["conv.weight"], sd["conv.weight"])
    fresh = Net(99).cuda()
    upd.copy_ema_to(fresh)
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, esd[k]), k
    # the optimizer's own state round-trips
    saved = upd.state_dict()
    other = optim.ParamUpdate(Net(4).cuda(), lr=1.0, ema_updates=0)
    other.load_state_dict(saved)
    assert torch.equal(other.exp_avg, upd.exp_avg) and torch.equal(other.exp_avg_sq, upd.exp_avg_sq)
    assert torch.equal(other.ema, upd.ema) and other.stats["step"].item() == 2
    assert other.stats["updates"].item() == UPDATES0 + 2
    with pytest.raises(TypeError):
        optim.ParamUpdate(Net(4).cuda().half(), lr=1e-3)
