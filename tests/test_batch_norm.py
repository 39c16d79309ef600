"""Synchronised batch norm with fused ReLU and residual (vampire_amd.norm over vamp_bn_*) against the
same formulas in float64 torch on the CPU, with autograd for the gradients, evaluated on the fp32 / 16-bit input values.

Bar, per tensor: err = max |x - x64|.  The HIP path may reach max(2 E_torch, 4 fp32 ulp of max |x64|), E_torch being
the same error of torch's own sequence (native_batch_norm + add + relu and its autograd) in the input's dtype on the
same GPU for the same inputs; a 16-bit output gets half a 16-bit ulp of the oracle value on top, element by element,
because it is rounded once.  Shapes are the smallest at which the kernels can still go wrong: every walk of a chunk
(flat, small planes, head / vectors / tail), one and several workgroups per channel, a channel that ends one element
past a split."""
import ctypes as C
import functools
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F
from torch import nn

from vampire_amd import _capi, _header, norm
from vampire_amd.build import build_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = norm.BN_CHUNK
EPS, MOM = 1e-5, 0.1
ULP4 = 4 * 2.0 ** -23
SHAPES = [(3, 5, 7, 9),            # odd planes: every plane starts off the 16-byte grid, head and tail loops run
          (2, 3, 1, 1),            # two elements per channel
          (1, 1, 1, 2),
          (2, 2048, 2, 3),         # many channels, tiny planes
          (2, 4, 3, 4),            # H W = 12: whole vectors in fp32, the small-plane walk in 16 bits
          (2, 3, 64, 100),         # 12800 per channel: four workgroups, the flat walk
          (1, 2, 17, 241),         # CH + 1 per channel: the second workgroup has one element
          (3, 2, 59, 71),          # odd planes of 4189 that straddle the splits, four workgroups
          (1, 257, 17, 241)]       # two chunks per channel AND more channels than the 256 threads of one merge
                                   # workgroup: the merges' second workgroup, one live thread in it (the c >= C guard)
assert 2 * 64 * 100 >= 3 * CH and 17 * 241 == CH + 1 and 3 * 59 * 71 >= 3 * CH
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
COMBOS = [(None, False), ("relu", False), (None, True), ("relu", True)]
gpu = pytest.mark.gpu


# =============================================================================================
# inputs, oracle, torch's own sequence, bar
# =============================================================================================
@functools.lru_cache(maxsize=None)
def make_case(shape, dtype, act, res, seed=0):
    """CPU tensors in the input's dtype, never modified.  With C >= 3: channel 0 is constant (0.75), channel 1 has
    mean 1000 and sigma 1 in fp32.  Under ReLU the constant channel's pre-activations are exactly 0: everywhere without
    a residual (bias 0), at every third position with one (residual = -bias).  dy holds exact zeros and negatives."""
    g = torch.Generator().manual_seed(seed + 17 * sum(shape))
    N, C_, H, W = shape
    mu, sigma = torch.randn(C_, generator=g) * 2, torch.rand(C_, generator=g) * 3 + 0.1
    x = mu.view(1, -1, 1, 1) + sigma.view(1, -1, 1, 1) * torch.randn(shape, generator=g)
    w, b = torch.randn(C_, generator=g) + 1.5, torch.randn(C_, generator=g)
    r = torch.randn(shape, generator=g) if res else None
    if C_ >= 3:
        x[:, 0] = 0.75
        if dtype == torch.float32:
            x[:, 1] = 1000.0 + torch.randn(N, H, W, generator=g)
        b[0] = 0.5 if res else 0.0
        if res:
            r[:, 0][(torch.arange(N * H * W) % 3 == 0).view(N, H, W)] = -0.5
    dy = torch.randn(shape, generator=g)
    dy[torch.rand(shape, generator=g) < 0.2] = 0.0
    rm, rv = torch.randn(C_, generator=g), torch.rand(C_, generator=g) + 0.5
    to = lambda t: None if t is None else t.to(dtype)
    return dict(x=to(x), w=w, b=b, r=to(r), dy=to(dy), rm=rm, rv=rv, act=act)


def formula(x, w, b, r, act, eps=EPS):
    """The operator in whatever dtype the arguments have: y, mean, invstd, biased variance."""
    mean = x.mean(dim=(0, 2, 3))
    var = ((x - mean.view(1, -1, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    v = w.view(1, -1, 1, 1) * (x - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)
    if r is not None:
        v = v + r
    return (torch.relu(v) if act == "relu" else v), mean, invstd, var


def running(rm, rv, mean, var, n, calls):
    out = []
    for _ in range(calls):
        rm = (1 - MOM) * rm + MOM * mean
        rv = (1 - MOM) * rv + MOM * var * n / (n - 1)
        out.append((rm, rv))
    return out


@functools.lru_cache(maxsize=None)
def oracle(shape, dtype, act, res):
    c = make_case(shape, dtype, act, res)
    x = c["x"].double().requires_grad_(True)
    w, b = c["w"].double().requires_grad_(True), c["b"].double().requires_grad_(True)
    r = c["r"].double().requires_grad_(True) if res else None
    y, mean, invstd, var = formula(x, w, b, r, act)
    leaves = [x, w, b] + ([r] if res else [])
    grads = torch.autograd.grad(y, leaves, c["dy"].double())
    n = shape[0] * shape[2] * shape[3]
    out = dict(y=y.detach(), mean=mean.detach(), invstd=invstd.detach(), dx=grads[0], gw=grads[1], gb=grads[2],
               gr=grads[3] if res else None)
    if n > 1:
        (out["rm1"], out["rv1"]), (out["rm2"], out["rv2"]) = running(c["rm"].double(), c["rv"].double(), out["mean"],
                                                                     var.detach(), n, 2)
    return out


def run_torch(c, dev):
    """torch's own sequence in the input's dtype on the GPU."""
    x = c["x"].to(dev).requires_grad_(True)
    w, b = c["w"].to(dev).requires_grad_(True), c["b"].to(dev).requires_grad_(True)
    r = c["r"].to(dev).requires_grad_(True) if c["r"] is not None else None
    rm, rv = c["rm"].to(dev), c["rv"].to(dev)
    v, mean, invstd = torch.native_batch_norm(x, w, b, rm, rv, True, MOM, EPS)
    if r is not None:
        v = v + r
    y = torch.relu(v) if c["act"] == "relu" else v
    leaves = [x, w, b] + ([r] if r is not None else [])
    grads = torch.autograd.grad(y, leaves, c["dy"].to(dev))
    out = dict(y=y.detach(), mean=mean, invstd=invstd, dx=grads[0], gw=grads[1], gb=grads[2],
               gr=grads[3] if r is not None else None, rm1=rm.clone(), rv1=rv.clone())
    torch.native_batch_norm(x.detach(), w.detach(), b.detach(), rm, rv, True, MOM, EPS)
    out["rm2"], out["rv2"] = rm, rv
    return out


def run_hip(c, dev):
    """The four functional steps at world size 1, twice forward (running statistics after one and two calls)."""
    x, w, b = c["x"].to(dev), c["w"].to(dev), c["b"].to(dev)
    r = c["r"].to(dev) if c["r"] is not None else None
    rm, rv, nbt = c["rm"].to(dev), c["rv"].to(dev), torch.zeros((), dtype=torch.int64, device=dev)
    rows = norm.gather_rows(norm.bn_partial_stats(x))
    y, saved = norm.bn_apply(x, rows, w, b, EPS, c["act"], r, rm, rv, MOM, nbt)
    out = dict(y=y, mean=saved[0], invstd=saved[1], rm1=rm.clone(), rv1=rv.clone(), saved=saved)
    y2, saved2 = norm.bn_apply(x, rows, w, b, EPS, c["act"], r, rm, rv, MOM, nbt)
    out.update(rm2=rm, rv2=rv, nbt=nbt, y2=y2, saved2=saved2, rows=rows)
    dy = c["dy"].to(dev)
    row, gw, gb = norm.bn_backward_partial(dy, x, y, saved, c["act"])
    dx, gr = norm.bn_backward_apply(dy, x, y, saved, w, norm.gather_rows(row), rows, c["act"], r is not None)
    out.update(dx=dx, gr=gr, gw=gw, gb=gb, brow=row)
    return out


def half_ulp16(ref, dtype):
    """Half a unit in the last place of dtype at |ref| (float64), element by element; 0 for fp32."""
    if dtype == torch.float32:
        return torch.zeros_like(ref)
    mant, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    e = torch.frexp(ref.abs().clamp_min(2.0 ** emin))[1].double() - 1          # floor(log2 |ref|)
    return 0.5 * torch.exp2(e - (mant - 1))


def check(label, got, own, ref, dtype=torch.float32):
    """`got` against the float64 `ref` under the bar; `own` is torch's result.  Returns err / bar (printed first)."""
    got, own = got.detach().double().cpu(), own.detach().double().cpu()
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    e_hip, e_own = float((got - ref).abs().max()), float((own - ref).abs().max())
    bar = max(2 * e_own, ULP4 * float(ref.abs().max()))
    tol = bar + half_ulp16(ref, dtype)
    frac = float(((got - ref).abs() / tol.clamp_min(2.0 ** -1000)).max())
    print(f"{label}: hip {e_hip:.3e}  torch {e_own:.3e}  bar {bar:.3e}  fraction {frac:.3f}")
    assert bool(((got - ref).abs() <= tol).all()), (label, e_hip, e_own, bar)
    return frac


@functools.lru_cache(maxsize=None)
def results(shape, dtype, act, res):
    c = make_case(shape, dtype, act, res)
    return c, oracle(shape, dtype, act, res), run_torch(c, "cuda"), run_hip(c, "cuda")


def _label(shape, dtype, act, res, name):
    return f"{shape} {str(dtype)[6:]} act={act} res={int(res)} {name}"


# =============================================================================================
# 1, 2: forward and backward against the oracle
# =============================================================================================
@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_against_the_oracle(shape, dtype):
    n = shape[0] * shape[2] * shape[3]
    for act, res in COMBOS:
        c, ref, own, hip = results(shape, dtype, act, res)
        lab = functools.partial(_label, shape, dtype, act, res)
        check(lab("y"), hip["y"], own["y"], ref["y"], dtype)
        check(lab("mean"), hip["mean"], own["mean"], ref["mean"])
        check(lab("invstd"), hip["invstd"], own["invstd"], ref["invstd"])
        # the float64 mean the backward takes is saved[0] + saved[2]
        assert float((hip["saved"][0].double() + hip["saved"][2].double()).cpu().sub(ref["mean"]).abs().max()) \
            <= 2.0 ** -40 * max(1.0, float(ref["mean"].abs().max()))
        if n > 1:
            for k in ("rm1", "rv1", "rm2", "rv2"):
                check(lab(k), hip[k], own[k], ref[k])
        assert int(hip["nbt"]) == 2
        assert torch.equal(hip["y"], hip["y2"]) and torch.equal(hip["saved"], hip["saved2"])
        assert float(hip["rows"][0, 0]) == n
        if shape[1] >= 3:                                       # the constant channel
            want = c["b"][0] + (c["r"][:, 0].float() if res else torch.zeros(shape[0], shape[2], shape[3]))
            want = (torch.relu(want) if act == "relu" else want).to(dtype)
            assert torch.equal(hip["y"][:, 0].cpu(), want), lab("constant channel")
            assert float(hip["rows"][0, 2]) == 0.0 and float(hip["rows"][0, 1]) == 0.75
            assert abs(float(hip["invstd"][0]) - EPS ** -0.5) <= ULP4 * EPS ** -0.5


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_against_float64_autograd(shape, dtype):
    for act, res in COMBOS:
        c, ref, own, hip = results(shape, dtype, act, res)
        lab = functools.partial(_label, shape, dtype, act, res)
        check(lab("dx"), hip["dx"], own["dx"], ref["dx"], dtype)
        check(lab("grad_weight"), hip["gw"], own["gw"], ref["gw"])
        check(lab("grad_bias"), hip["gb"], own["gb"], ref["gb"])
        if res:
            check(lab("grad_residual"), hip["gr"], own["gr"], ref["gr"], dtype)
            # dz is dy or 0, bit for bit, and 0 wherever the output is 0
            dy = c["dy"].to("cuda")
            want = torch.where(hip["y"] > 0, dy, torch.zeros_like(dy)) if act == "relu" else dy
            assert torch.equal(hip["gr"], want), lab("grad_residual bits")
            if act == "relu" and shape[1] >= 3:
                zero = hip["y"][:, 0] == 0
                assert int(zero.sum()) >= 1 and bool((hip["gr"][:, 0][zero] == 0).all())
        elif act == "relu" and shape[1] >= 3:                   # every pre-activation of channel 0 is exactly 0
            assert float(hip["gb"][0]) == 0.0 and float(hip["gw"][0]) == 0.0


def _evaluation_mode(shapes, dtype):
    for shape in shapes:
        for act, res in COMBOS:
            c = make_case(shape, dtype, act, res)
            dev = "cuda"
            def run(t, where):
                cast = (lambda v: v.double()) if t else (lambda v: v)
                v = F.batch_norm(cast(c["x"]).to(where), cast(c["rm"]).to(where), cast(c["rv"]).to(where),
                                 cast(c["w"]).to(where), cast(c["b"]).to(where), False, MOM, EPS)
                v = v + cast(c["r"]).to(where) if res else v
                return torch.relu(v) if act == "relu" else v
            rm, rv = c["rm"].to(dev), c["rv"].to(dev)
            y = norm.bn_apply_eval(c["x"].to(dev), c["w"].to(dev), c["b"].to(dev), rm, rv, EPS, act,
                                   c["r"].to(dev) if res else None)
            check(_label(shape, dtype, act, res, "eval y"), y, run(False, dev), run(True, "cpu"), dtype)
            assert torch.equal(rm.cpu(), c["rm"]) and torch.equal(rv.cpu(), c["rv"])


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_evaluation_mode_against_float64_batch_norm(dtype):
    _evaluation_mode([(3, 5, 7, 9), (2, 3, 64, 100)], dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", SHAPES + [(1, 3, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_evaluation_mode_over_every_shape(shape, dtype):
    """Every walk of a chunk, one and several chunks per channel, and the one value per channel that evaluation mode
    accepts and training refuses; the running statistics stay as they were."""
    _evaluation_mode([shape], dtype)


@gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (1, 2, 17, 241)], ids=lambda s: "x".join(map(str, s)))
def test_training_without_running_statistics_or_counter(shape, dtype):
    """update_running = 0 and no batch counter: y and saved have the bits of the call that has them."""
    for act, res in COMBOS:
        c, _, _, hip = results(shape, dtype, act, res)
        y, saved = norm.bn_apply(c["x"].to("cuda"), hip["rows"], c["w"].to("cuda"), c["b"].to("cuda"), EPS, act,
                                 c["r"].to("cuda") if res else None)
        assert torch.equal(y, hip["y"]) and torch.equal(saved, hip["saved"]), _label(shape, dtype, act, res, "bits")


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d)[6:])
def test_merge_kernels_write_every_channel_of_their_rows(dtype):
    """C = 257 with two chunks per channel, into rows and gradients that hold NaN beforehand: the second workgroup of
    bn_merge_stats_kernel / bn_merge_bwd_kernel writes channel 256, and the rows have the bits of the wrappers' own."""
    shape, dev = (1, 257, 17, 241), "cuda"
    c, _, _, hip = results(shape, dtype, "relu", True)
    x, dy = c["x"].to(dev), c["dy"].to(dev)
    vamp, nan = _capi.checked(), float("nan")
    d = norm._desc(x)
    ws = norm.scratch("batch_norm", x.device, vamp.vamp_bn_workspace_bytes(d))
    row = torch.full((2 * shape[1] + 1,), nan, dtype=torch.float64, device=dev)
    vamp.vamp_bn_partial_stats(d, x, row, ws, ws.numel(), norm._stream())
    assert torch.equal(row, hip["rows"][0]), "the forward's row"
    brow = torch.full((2 * shape[1],), nan, dtype=torch.float64, device=dev)
    gw, gb = (torch.full((shape[1],), nan, device=dev) for _ in range(2))
    vamp.vamp_bn_backward_partial(norm._desc(x, "relu"), dy, x, hip["y"], hip["saved"], brow, gw, gb, ws, ws.numel(),
                                  norm._stream())
    for what, got, want in (("row", brow, hip["brow"]), ("grad_weight", gw, hip["gw"]), ("grad_bias", gb, hip["gb"])):
        assert torch.equal(got, want), f"the backward's {what}"


def _poisoned(dtype, act, where):
    """(2, 4, 7, 9): channel 0 holds one NaN, channel 1 one +inf -- at the channel's first element (the pivot of the
    statistics' sums) or inside its second plane -- and channels 2 and 3 are clean.  The case and its clean twin."""
    clean = make_case((2, 4, 7, 9), dtype, act, False)
    x = clean["x"].clone()
    n, h, w = (0, 0, 0) if where == "first" else (1, 3, 5)
    x[n, 0, h, w], x[n, 1, h, w] = float("nan"), float("inf")
    return dict(clean, x=x), clean


@gpu
@pytest.mark.parametrize("where", ["first", "inner"])
@pytest.mark.parametrize("act", [None, "relu"], ids=["none", "relu"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d)[6:])
def test_non_finite_inputs_stay_in_their_channel(dtype, act, where):
    """The file comment's two claims: "a NaN stays" (through max(M2, 0) and through the ReLU, as torch.relu keeps it)
    and "a mean of +-inf: inf - inf" (the low word of such a mean is 0, not NaN).  The NaN masks of y, mean and invstd
    are those of torch's own sequence on the device and of the float64 formula; the clean channels have the bits of
    the run in which no channel is poisoned."""
    dev = "cuda"
    c, clean = _poisoned(dtype, act, where)
    hip, hip_clean, own = run_hip(c, dev), run_hip(clean, dev), run_torch(c, dev)
    y64, mean64, invstd64, _ = formula(c["x"].double(), c["w"].double(), c["b"].double(), None, act)
    for k, ref in (("y", y64), ("mean", mean64), ("invstd", invstd64)):
        got, tor, want = (t.detach().cpu().isnan() for t in (hip[k], own[k], ref))
        print(f"(2, 4, 7, 9) {str(dtype)[6:]} act={act} poison={where} {k}: NaN in hip {int(got.sum())}, torch "
              f"{int(tor.sum())}, float64 {int(want.sum())} of {got.numel()}; mean of the inf channel: hip "
              f"{float(hip['mean'][1])}, torch {float(own['mean'][1])}, float64 {float(mean64[1])}")
        assert torch.equal(got, want), f"{k}: NaN mask differs from the float64 formula's"
        assert torch.equal(got, tor), f"{k}: NaN mask differs from torch's own"
    assert bool(hip["y"][:, :2].isnan().all()) and not bool(hip["y"][:, 2:].isnan().any())
    for k in ("y", "y2"):
        assert torch.equal(hip[k][:, 2:], hip_clean[k][:, 2:]), k
    for k in ("saved", "saved2"):
        assert torch.equal(hip[k][:, 2:], hip_clean[k][:, 2:]), k
    for k in ("rm1", "rv1", "rm2", "rv2"):
        assert torch.equal(hip[k][2:], hip_clean[k][2:]), k
    assert torch.equal(hip["rows"][0, 5:], hip_clean["rows"][0, 5:]) and int(hip["nbt"]) == 2


# =============================================================================================
# 3: two ranks on one GPU
# =============================================================================================
@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape", [(5, 4, 7, 9), (5, 2, 40, 52)], ids=lambda s: "x".join(map(str, s)))
def test_two_ranks_on_one_gpu(shape, dtype):
    act, res, dev = "relu", True, "cuda"
    c, ref = make_case(shape, dtype, act, res), oracle(shape, dtype, act, res)
    own = run_torch(c, dev)
    halves = [slice(0, 3), slice(3, 5)]
    x, r, dy = c["x"].to(dev), c["r"].to(dev), c["dy"].to(dev)
    w, b = c["w"].to(dev), c["b"].to(dev)

    def both(order):
        rows = torch.stack([norm.bn_partial_stats(x[h]) for h in halves])[order]
        outs = []
        for h in halves:
            rm, rv = c["rm"].to(dev), c["rv"].to(dev)
            y, saved = norm.bn_apply(x[h], rows, w, b, EPS, act, r[h], rm, rv, MOM)
            outs.append(dict(y=y, saved=saved, rm=rm, rv=rv))
        for h, o in zip(halves, outs):
            o["brow"], o["gw"], o["gb"] = norm.bn_backward_partial(dy[h], x[h], o["y"], o["saved"], act)
        brows = torch.stack([o["brow"] for o in outs])[order]
        for h, o in zip(halves, outs):
            o["dx"], o["gr"] = norm.bn_backward_apply(dy[h], x[h], o["y"], o["saved"], w, brows, rows, act, True)
        return outs

    lab = functools.partial(_label, shape, dtype, act, res)
    for order, tag in (([0, 1], "two ranks"), ([1, 0], "rows swapped")):
        a, bb = both(order)
        cat = lambda k: torch.cat([a[k], bb[k]])
        check(lab(f"{tag} y"), cat("y"), own["y"], ref["y"], dtype)
        check(lab(f"{tag} dx"), cat("dx"), own["dx"], ref["dx"], dtype)
        check(lab(f"{tag} grad_residual"), cat("gr"), own["gr"], ref["gr"], dtype)
        check(lab(f"{tag} mean"), a["saved"][0], own["mean"], ref["mean"])
        check(lab(f"{tag} invstd"), a["saved"][1], own["invstd"], ref["invstd"])
        check(lab(f"{tag} running_mean"), a["rm"], own["rm1"], ref["rm1"])
        check(lab(f"{tag} running_var"), a["rv"], own["rv1"], ref["rv1"])
        for k in ("saved", "rm", "rv"):
            assert torch.equal(a[k], bb[k]), (tag, k)
        check(lab(f"{tag} grad_weight"), a["gw"].double() + bb["gw"].double(), own["gw"], ref["gw"])
        check(lab(f"{tag} grad_bias"), a["gb"].double() + bb["gb"].double(), own["gb"], ref["gb"])


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("shape,sizes", [((64, 3, 2, 3), (1,) * 64),       # the most ranks the contract allows
                                         ((7, 3, 5, 7), (1, 2, 4)),        # unequal ranks
                                         ((3, 2, 1, 1), (1, 1, 1))],       # every rank: n = 1 and M2 = 0 exactly
                         ids=["64-ranks", "ranks-of-1-2-4", "one-element-ranks"])
def test_many_and_unequal_ranks_on_one_gpu(shape, sizes, dtype):
    """The rank loops of bn_apply_kernel and bn_bwd_apply_kernel past their second trip, with ranks of unequal size,
    and with ranks of one element per channel, where Chan's merge does all the work: relu + residual against the
    float64 oracle of the whole batch, rows in rank order and in one permuted order (every rank sees the same rows,
    so saved and running statistics are bit-equal on all of them in either order)."""
    act, res, dev = "relu", True, "cuda"
    c, ref = make_case(shape, dtype, act, res), oracle(shape, dtype, act, res)
    own = run_torch(c, dev)
    world, starts = len(sizes), [sum(sizes[:k]) for k in range(len(sizes))]
    parts = [slice(s, s + n) for s, n in zip(starts, sizes)]
    assert starts[-1] + sizes[-1] == shape[0]
    x, r, dy = c["x"].to(dev), c["r"].to(dev), c["dy"].to(dev)
    w, b = c["w"].to(dev), c["b"].to(dev)

    def ranks(order):
        own_rows = [norm.bn_partial_stats(x[h]) for h in parts]
        if shape[2] * shape[3] == 1:
            for row in own_rows:                                # one element per channel: n = 1, M2 = 0
                assert float(row[0]) == 1.0 and bool((row[2::2] == 0).all())
        rows = torch.stack(own_rows)[order]
        outs = []
        for h in parts:
            rm, rv = c["rm"].to(dev), c["rv"].to(dev)
            y, saved = norm.bn_apply(x[h], rows, w, b, EPS, act, r[h], rm, rv, MOM)
            outs.append(dict(y=y, saved=saved, rm=rm, rv=rv))
        for h, o in zip(parts, outs):
            o["brow"], o["gw"], o["gb"] = norm.bn_backward_partial(dy[h], x[h], o["y"], o["saved"], act)
        brows = torch.stack([o["brow"] for o in outs])[order]
        for h, o in zip(parts, outs):
            o["dx"], o["gr"] = norm.bn_backward_apply(dy[h], x[h], o["y"], o["saved"], w, brows, rows, act, True)
        return outs

    lab = functools.partial(_label, shape, dtype, act, res)
    permuted = [(5 * i + 3) % world for i in range(world)]
    assert sorted(permuted) == list(range(world)) and permuted != list(range(world))
    for order, tag in ((list(range(world)), f"{world} ranks"), (permuted, f"{world} ranks, rows permuted")):
        outs = ranks(order)
        cat = lambda k: torch.cat([o[k] for o in outs])
        check(lab(f"{tag} y"), cat("y"), own["y"], ref["y"], dtype)
        check(lab(f"{tag} dx"), cat("dx"), own["dx"], ref["dx"], dtype)
        check(lab(f"{tag} grad_residual"), cat("gr"), own["gr"], ref["gr"], dtype)
        check(lab(f"{tag} mean"), outs[0]["saved"][0], own["mean"], ref["mean"])
        check(lab(f"{tag} invstd"), outs[0]["saved"][1], own["invstd"], ref["invstd"])
        check(lab(f"{tag} running_mean"), outs[0]["rm"], own["rm1"], ref["rm1"])
        check(lab(f"{tag} running_var"), outs[0]["rv"], own["rv1"], ref["rv1"])
        for o in outs[1:]:
            for k in ("saved", "rm", "rv"):
                assert torch.equal(outs[0][k], o[k]), (tag, k)
        total = lambda k: torch.stack([o[k].double() for o in outs]).sum(0)
        check(lab(f"{tag} grad_weight"), total("gw"), own["gw"], ref["gw"])
        check(lab(f"{tag} grad_bias"), total("gb"), own["gb"], ref["gb"])


# =============================================================================================
# 4: repeatable and capturable
# =============================================================================================
@gpu
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 3, 64, 100)], ids=lambda s: "x".join(map(str, s)))
def test_same_call_twice_gives_equal_bits(shape):
    for dtype in (torch.float32, torch.float16):
        c = make_case(shape, dtype, "relu", True)
        a, b = run_hip(c, "cuda"), run_hip(c, "cuda")
        for k in ("y", "saved", "rm1", "rv1", "rm2", "rv2", "nbt", "rows", "brow", "dx", "gr", "gw", "gb"):
            assert torch.equal(a[k], b[k]), (shape, dtype, k)


@gpu
def test_module_forward_backward_replays_in_a_graph():
    shape, dev = (2, 3, 64, 100), "cuda"
    first, second = make_case(shape, torch.float32, "relu", True), make_case(shape, torch.float32, "relu", True, seed=5)
    mod = norm.BatchNormAct2d(shape[1], act="relu").to(dev)
    with torch.no_grad():
        mod.weight.copy_(first["w"]), mod.bias.copy_(first["b"])
    xs, rs, dys = (first[k].to(dev).clone() for k in ("x", "r", "dy"))
    xs.requires_grad_(True), rs.requires_grad_(True)
    leaves = [xs, rs, mod.weight, mod.bias]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                               # (warm-up: workspaces exist before the capture)
        torch.autograd.grad(mod(xs, rs), leaves, dys)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = mod(xs, rs)
        gs = torch.autograd.grad(ys, leaves, dys)
    with torch.no_grad():
        for dst, k in ((xs, "x"), (rs, "r"), (dys, "dy")):
            dst.copy_(second[k].to(dev))
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    graph.replay()
    torch.cuda.synchronize()
    eager = norm.BatchNormAct2d(shape[1], act="relu").to(dev)
    eager.load_state_dict(state)
    xe, re_ = second["x"].to(dev).requires_grad_(True), second["r"].to(dev).requires_grad_(True)
    ye = eager(xe, re_)
    ge = torch.autograd.grad(ye, [xe, re_, eager.weight, eager.bias], second["dy"].to(dev))
    assert torch.equal(ys, ye)
    for a, b in zip(gs, ge):
        assert torch.equal(a, b)
    for k, v in eager.state_dict().items():
        assert torch.equal(mod.state_dict()[k], v), k
    assert int(mod.num_batches_tracked) == int(state["num_batches_tracked"]) + 1 == 2


# =============================================================================================
# 5: the encoders
# =============================================================================================
def _model_run(model, inputs, ups, train=True):
    """Outputs, parameter gradients and running statistics of one forward (+ backward under `train`)."""
    model.train(train)
    outs = model(*inputs)
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    if train:
        params = [p for p in model.parameters()]
        grads = torch.autograd.grad(outs, params, [u.to(o) for u, o in zip(ups, outs)])
        res.update({f"grad {n}": g for (n, _), g in zip(model.named_parameters(), grads)})
        res.update({f"buf {n}": b.detach().clone() for n, b in model.named_buffers() if b.dtype.is_floating_point})
    return res


def _encoder_cases():
    """The bottleneck stack is 8 channels wide at its base.  At 64, one of its 2.6 M ReLU inputs lies within fp32
    rounding of zero in float64, and which side an fp32 run puts it on decides errors of 1e-3 of scale in most
    parameter gradients: torch's own fp32 model on the CPU then misses the float64 gradients by the same amounts as
    the HIP path on the GPU (grad layer1.0.downsample.1.weight 2.659 and 2.660, bn2.weight 4.077 both), while the
    default fp32 model on the GPU, with its own roundings, drew 0.29 there -- a draw between fp32 roundings, not a
    property of either operator.  Eight times fewer elements make such an element unlikely (none in the fp32 CPU
    run; gradient errors 1e-6 of scale), and every kernel path runs as before.  The 64-wide stack is still run
    (`bottleneck64`) for everything a single sign cannot move: outputs and running statistics in training mode,
    outputs in evaluation mode.  `resnet18-converted` is the default model after convert_batch_norm."""
    from vampire_amd.encoders import ResNet, SECONDFPN
    g = torch.Generator().manual_seed(11)
    img = torch.randn(3, 3, 64, 96, generator=g)
    feats = [torch.randn(3, 16, 16, 24, generator=g), torch.randn(3, 32, 8, 12, generator=g)]
    sync = dict(type="SyncBN")
    return {"resnet18": (lambda nc: ResNet(depth=18, norm_cfg=nc), sync, (img,)),
            "bottleneck": (lambda nc: ResNet(depth=50, num_stages=2, strides=(1, 2), dilations=(1, 1),
                                             out_indices=(0, 1), base_channels=8, norm_cfg=nc), sync, (img,)),
            "bottleneck64": (lambda nc: ResNet(depth=50, num_stages=2, strides=(1, 2), dilations=(1, 1),
                                               out_indices=(0, 1), norm_cfg=nc), sync, (img,)),
            "resnet18-converted": (lambda nc: ResNet(depth=18) if nc is None
                                   else norm.convert_batch_norm(ResNet(depth=18)), sync, (img,)),
            "secondfpn": (lambda nc: SECONDFPN([16, 32], [8, 8], [1, 2], norm_cfg=nc),
                          dict(type="SyncBN", eps=1e-3, momentum=0.01), (feats,))}


@gpu
@pytest.mark.parametrize("name", ["resnet18", "bottleneck", "bottleneck64", "resnet18-converted", "secondfpn"])
def test_encoders_with_sync_bn_match_the_default_models(name):
    build, cfg, inputs = _encoder_cases()[name]
    torch.manual_seed(3)
    default = build(None)
    with torch.no_grad():                                       # statistics and affine terms away from their defaults
        for m in default.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5), m.bias.normal_(0, 0.2)
                m.running_mean.normal_(0, 0.1), m.running_var.uniform_(0.5, 1.5)
    state = {k: v.clone() for k, v in default.state_dict().items()}
    fused = build(cfg)
    assert set(fused.state_dict()) == set(state)
    assert [n for n, _ in fused.named_modules()] == [n for n, _ in default.named_modules()]
    acts = {m.act for m in fused.modules() if isinstance(m, norm.BatchNormAct2d)}
    assert acts == ({None} if name.endswith("converted") else {"relu"} if name == "secondfpn" else {None, "relu"})
    assert not any(type(m) is nn.BatchNorm2d for m in fused.modules())
    fused.load_state_dict(state)
    default.load_state_dict(fused.state_dict())
    move = lambda args, f: tuple([f(t) for t in a] if isinstance(a, list) else f(a) for a in args)
    g = torch.Generator().manual_seed(5)
    for train in (True, False):
        ref_model = build(None).double()
        ref_model.load_state_dict(state)
        with torch.no_grad():                                   # (shapes of the outputs, for the upstream gradients)
            shapes = [o.shape for o in build(None).eval()(*inputs)]
        ups = [torch.randn(sh, generator=g) for sh in shapes]
        ref = _model_run(ref_model, move(inputs, lambda t: t.double()), ups, train)
        d32, f32 = build(None).cuda(), build(cfg).cuda()
        d32.load_state_dict(state), f32.load_state_dict(state)
        own = _model_run(d32, move(inputs, lambda t: t.cuda()), ups, train)
        got = _model_run(f32, move(inputs, lambda t: t.cuda()), ups, train)
        assert set(got) == set(ref)
        for k in ref:
            if name == "bottleneck64" and k.startswith("grad "):
                continue                                        # (see _encoder_cases: checked 8 channels wide)
            check(f"{name} train={train} {k}", got[k], own[k], ref[k].cpu())


# =============================================================================================
# 6: contract
# =============================================================================================
@gpu
def test_refusals_raise_with_their_messages():
    with pytest.raises(ValueError, match="momentum=None"):
        norm.BatchNormAct2d(4, momentum=None)
    with pytest.raises(ValueError, match="affine=False"):
        norm.BatchNormAct2d(4, affine=False)
    with pytest.raises(ValueError, match="track_running_stats=False"):
        norm.BatchNormAct2d(4, track_running_stats=False)
    with pytest.raises(ValueError, match="act must be"):
        norm.BatchNormAct2d(4, act="gelu")
    mod = norm.BatchNormAct2d(4, act="relu").cuda()
    x = torch.randn(2, 4, 3, 5, device="cuda")
    with pytest.raises(_capi.VampireHipError, match="device tensor"):
        mod(x.cpu())
    with pytest.raises(ValueError, match="4-D"):
        mod(x[0])
    with pytest.raises(ValueError, match="residual must have x's shape and dtype"):
        mod(x, x[:1])
    with pytest.raises(ValueError, match="residual must have x's shape and dtype"):
        mod(x, x.half())
    with pytest.raises(ValueError, match="N H W == 1"):
        mod(x[:1, :, :1, :1])
    mod.eval()
    y = mod(x[:1, :, :1, :1].requires_grad_(True))            # evaluation takes one value per channel ...
    with pytest.raises(NotImplementedError, match="evaluation mode"):
        y.sum().backward()                                      # ... and has no backward
    with pytest.raises(TypeError, match="fp32, bf16 or fp16"):
        norm.bn_partial_stats(x.double())
    with pytest.raises(ValueError, match="float64 rows"):
        norm.bn_apply(x, torch.zeros(1, 9, device="cuda"), mod.weight, mod.bias)
    with pytest.raises(ValueError, match="ranks"):
        norm.bn_apply(x, torch.zeros(65, 9, dtype=torch.float64, device="cuda"), mod.weight, mod.bias)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=lambda d: str(d)[6:])
def test_channels_last_input_gives_the_bits_of_its_contiguous_copy(dtype):
    c = make_case((3, 5, 7, 9), dtype, "relu", True)
    outs = []
    for fmt in (torch.contiguous_format, torch.channels_last):
        mod = norm.BatchNormAct2d(5, act="relu").cuda()
        with torch.no_grad():
            mod.weight.copy_(c["w"]), mod.bias.copy_(c["b"])
        x = c["x"].cuda().contiguous(memory_format=fmt).requires_grad_(True)
        r = c["r"].cuda().contiguous(memory_format=fmt).requires_grad_(True)
        y = mod(x, r)
        gs = torch.autograd.grad(y, [x, r, mod.weight, mod.bias], c["dy"].cuda().contiguous(memory_format=fmt))
        outs.append([y, *gs, mod.running_mean, mod.running_var])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # a view that starts off the 16-byte grid is copied, too
    base = torch.zeros(c["x"].numel() + 1, dtype=dtype, device="cuda")
    base[1:] = c["x"].cuda().view(-1)
    odd = base[1:].view(c["x"].shape)
    assert odd.data_ptr() % 16 != 0
    assert torch.equal(norm.bn_partial_stats(odd), norm.bn_partial_stats(c["x"].cuda()))


@gpu
def test_convert_batch_norm_keeps_tensors_and_values():
    def build():
        return nn.Sequential(nn.Conv2d(3, 6, 3, padding=1), nn.BatchNorm2d(6, eps=1e-3, momentum=0.2), nn.ReLU(),
                             nn.Sequential(nn.Conv2d(6, 4, 1), nn.BatchNorm2d(4)))
    torch.manual_seed(2)
    model, own_model, ref_model = build().cuda(), build().cuda(), build().double()
    own_model.load_state_dict(model.state_dict())
    ref_model.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    x = torch.randn(4, 3, 9, 11, device="cuda")
    before = {k: v.data_ptr() for k, v in model.state_dict(keep_vars=True).items()}
    values = {k: v.clone() for k, v in model.state_dict().items()}
    assert norm.convert_batch_norm(model) is model
    assert type(model[1]) is norm.BatchNormAct2d and type(model[3][1]) is norm.BatchNormAct2d
    assert model[1].act is None and model[1].eps == 1e-3 and model[1].momentum == 0.2 and model[1].training
    assert {k: v.data_ptr() for k, v in model.state_dict(keep_vars=True).items()} == before
    for k, v in model.state_dict().items():
        assert torch.equal(v, values[k]), k
    got, own, ref = model(x), own_model(x), ref_model(x.double().cpu())
    check("converted model output", got, own, ref.detach())
    for k, v in model.state_dict().items():
        if "running" in k:
            check(f"converted model {k}", v, own_model.state_dict()[k], ref_model.state_dict()[k])
    assert int(model[1].num_batches_tracked) == 1
    lone = norm.convert_batch_norm(nn.BatchNorm2d(3).eval())
    assert type(lone) is norm.BatchNormAct2d and not lone.training and not norm.is_fused(lone)


@gpu
def test_converted_norm_in_front_of_an_inplace_relu_runs_its_backward():
    """Models built elsewhere follow the norm with an in-place ReLU: a bare norm must not keep its output for the
    backward (autograd would refuse the modified tensor).  Values and gradients against the unconverted model."""
    def build():
        return nn.Sequential(nn.Conv2d(3, 6, 3, padding=1, bias=False), nn.BatchNorm2d(6), nn.ReLU(inplace=True),
                             nn.Conv2d(6, 4, 1, bias=False), nn.BatchNorm2d(4), nn.ReLU(inplace=True))
    torch.manual_seed(4)
    own_model, ref_model = build().cuda(), build().double()
    ref_model.load_state_dict({k: v.cpu() for k, v in own_model.state_dict().items()})
    model = norm.convert_batch_norm(build().cuda())
    model.load_state_dict(own_model.state_dict())
    g = torch.Generator().manual_seed(6)
    x, up = torch.randn(4, 3, 9, 11, generator=g), torch.randn(4, 4, 9, 11, generator=g)
    res = {}
    for key, m, cast in (("got", model, lambda t: t.cuda()), ("own", own_model, lambda t: t.cuda()),
                         ("ref", ref_model, lambda t: t.double())):
        y = m(cast(x))
        grads = torch.autograd.grad(y, list(m.parameters()), cast(up))
        res[key] = [y.detach()] + list(grads)
    names = ["output"] + [f"grad {n}" for n, _ in model.named_parameters()]
    for n, got, own, ref in zip(names, res["got"], res["own"], res["ref"]):
        check(f"inplace relu {n}", got, own, ref)


# =============================================================================================
# CPU tests
# =============================================================================================
def _gather_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from vampire_amd.norm import gather_rows
    dist.init_process_group("gloo", rank=rank, world_size=world)
    g = torch.Generator().manual_seed(100 + rank)
    row = torch.randn(11, dtype=torch.float64, generator=g)
    rows = gather_rows(row, dist.group.WORLD)
    out[rank] = (row.view(torch.int64).tolist(), rows.view(torch.int64).tolist(), tuple(rows.shape))
    dist.destroy_process_group()


def test_gather_rows_in_two_gloo_ranks():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_gather_worker, args=(2, port, out), nprocs=2, join=True)
    assert out[0][2] == out[1][2] == (2, 11)
    assert out[0][0] != out[1][0]
    for rank in (0, 1):
        assert out[rank][1] == [out[0][0], out[1][0]]           # rank order, bit for bit, on both ranks
    row = torch.arange(5, dtype=torch.float64)
    alone = norm.gather_rows(row)
    assert alone.shape == (1, 5) and alone.data_ptr() == row.data_ptr()


def test_defaults_construct_todays_modules():
    from vampire_amd import encoders, multitask
    from vampire_amd.config import CFG_TINY
    assert type(norm.build_norm(None, 8)) is nn.BatchNorm2d
    bn = norm.build_norm(dict(type="BN", eps=1e-3, momentum=0.01), 8, act="relu")
    assert type(bn) is nn.BatchNorm2d and bn.eps == 1e-3 and bn.momentum == 0.01
    sb = norm.build_norm(dict(type="SyncBN", eps=1e-3, momentum=0.01), 8, act="relu")
    assert type(sb) is norm.BatchNormAct2d and (sb.eps, sb.momentum, sb.act) == (1e-3, 0.01, "relu")
    assert set(sb.state_dict()) == set(bn.state_dict())
    with pytest.raises(ValueError, match="norm_cfg type"):
        norm.build_norm(dict(type="GN"), 8)
    bc, hc = multitask.reference_confs(CFG_TINY, small_encoder=True)
    assert (bc, hc) == multitask.reference_confs(CFG_TINY, small_encoder=True, norm="BN")
    assert "norm_cfg" not in bc["img_backbone_conf"] and "norm_cfg" not in hc
    bs, hs = multitask.reference_confs(CFG_TINY, small_encoder=True, norm="SyncBN")
    for conf in (bs["img_backbone_conf"], bs["img_neck_conf"], hs["bev_backbone_conf"], hs["bev_neck_conf"], hs):
        assert conf["norm_cfg"]["type"] == "SyncBN"
    with pytest.raises(ValueError, match="norm must be"):
        multitask.reference_confs(CFG_TINY, norm="GN")
    models = [encoders.ResNet(depth=18), encoders.ResNet(depth=50, num_stages=2),
              encoders.SECONDFPN([16, 32], [8, 8], [1, 2]), encoders.SECONDFPN([16, 32], [8, 8], [0.5, 1]),
              multitask.BEVDepthHead(**hc)]
    for m in models:
        kinds = {type(c) for c in m.modules()}
        assert norm.BatchNormAct2d not in kinds and nn.Identity not in kinds and nn.BatchNorm2d in kinds
        assert nn.ReLU in kinds or isinstance(m, encoders.ResNet)
    assert isinstance(models[0].relu, nn.ReLU) and isinstance(models[2].deblocks[0][2], nn.ReLU)
    keys = list(models[0].state_dict())
    assert keys[:6] == ["conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var",
                        "bn1.num_batches_tracked"]
    assert "layer2.0.downsample.1.running_var" in keys and "layer1.1.bn2.weight" in keys
    assert list(models[2].state_dict())[:3] == ["deblocks.0.0.weight", "deblocks.0.1.weight", "deblocks.0.1.bias"]
    fused_head = multitask.BEVDepthHead(**hs)
    assert list(fused_head.state_dict()) == list(models[4].state_dict())
    assert not any(type(c) is nn.BatchNorm2d for c in fused_head.modules())
    x = torch.randn(2, 3, 32, 32)
    assert [o.shape for o in models[0].eval()(x)] == [o.shape for o in encoders.ResNet(depth=18).eval()(x)]


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _good_desc():
    return _capi.VampBatchNormDesc(eps=1e-5, momentum=0.1, N=2, C=3, H=4, W=5, dtype=_capi.VAMP_F32,
                                   act=_capi.VAMP_BN_ACT_RELU, has_residual=0, training=1, world=1, update_running=0)


def _entry_calls(lib, d):
    """Every vamp_bn_* launcher with NULL pointers: (name, return code)."""
    nul = [None]
    return [("vamp_bn_partial_stats", lib.vamp_bn_partial_stats(d, None, None, None, 0, None)),
            ("vamp_bn_apply", lib.vamp_bn_apply(d, *(nul * 10), None)),
            ("vamp_bn_backward_partial", lib.vamp_bn_backward_partial(d, *(nul * 7), None, 0, None)),
            ("vamp_bn_backward_apply", lib.vamp_bn_backward_apply(d, *(nul * 9), None))]


@pytest.mark.parametrize("field,value,message", [
    ("C", 0, b"C must be at least 1"), ("N", 0, b"N, H and W must be at least 1"),
    ("H", 1 << 30, b"N H W must be below 2^31"), ("world", 0, b"world must be in 1 .. 64"),
    ("world", 65, b"world must be in 1 .. 64"), ("dtype", 7, b"dtype must be"), ("act", 2, b"act must be"),
    ("has_residual", 2, b"has_residual must be"), ("training", -1, b"training must be"),
    ("eps", -1.0, b"eps must not be negative"), ("momentum", 1.5, b"momentum must be")])
def test_bad_descriptor_fields_are_refused_without_gpu(lib, field, value, message):
    d = _good_desc()
    assert lib.vamp_bn_workspace_bytes(d) > 0
    setattr(d, field, value)
    assert lib.vamp_bn_workspace_bytes(d) == 0
    assert message in lib.vamp_last_error()
    for name, rc in _entry_calls(lib, d):
        assert rc == -1, name
    lib.vamp_bn_apply(d, *([None] * 11))
    assert message in lib.vamp_last_error()


def test_bad_pointers_are_refused_without_gpu(lib):
    d = _good_desc()
    for name, rc in _entry_calls(lib, d):                       # a good descriptor stops at the pointer checks
        assert rc == -1, name
        assert b"NULL" in lib.vamp_last_error(), name
    d.has_residual = 1
    assert lib.vamp_bn_apply(d, *([None] * 11)) == -1
    assert b"has_residual is set but residual is NULL" in lib.vamp_last_error()
    assert lib.vamp_bn_backward_apply(d, *([None] * 10)) == -1
    assert b"has_residual is set but grad_residual is NULL" in lib.vamp_last_error()
    d.has_residual = 0
    # host addresses stand in for device memory: every call below is refused before any launch
    buf = C.create_string_buffer(4096)
    a = (C.addressof(buf) + 15) // 16 * 16
    assert lib.vamp_bn_partial_stats(d, a, a + 4, a, 4096, None) == -1
    assert b"float64 row must be 8-byte aligned" in lib.vamp_last_error()
    assert lib.vamp_bn_apply(d, a, None, a + 4, a, a, None, None, None, a, a, None) == -1
    assert b"float64 rows must be 8-byte aligned" in lib.vamp_last_error()
    assert lib.vamp_bn_apply(d, a + 4, None, a, a, a, None, None, None, a, a, None) == -1
    assert b"16-byte aligned" in lib.vamp_last_error()
    assert lib.vamp_bn_backward_apply(d, a, a, a, a, a, a + 4, a, a, None, None) == -1
    assert b"float64 rows must be 8-byte aligned" in lib.vamp_last_error()
    assert lib.vamp_bn_partial_stats(d, a, a, a, 8, None) == -2
    assert b"workspace 8 <" in lib.vamp_last_error()
    d.training = 0
    assert lib.vamp_bn_backward_partial(d, *([None] * 7), None, 0, None) == -1
    assert b"evaluation mode has no backward" in lib.vamp_last_error()


def test_library_exports_every_bn_symbol(lib):
    header = _header.read()
    names = sorted(n for n in header.prototypes if n.startswith("vamp_bn_"))
    assert names ==["vamp_bn_apply", "vamp_bn_backward_apply", "vamp_bn_backward_partial", "vamp_bn_partial_stats",
                     "vamp_bn_workspace_bytes"]
    raw = C.CDLL(_capi.lib_path())
    for n in names:
        assert hasattr(raw, n) and n in _capi.SIGNATURES, n
    assert C.sizeof(_capi.VampBatchNormDesc) == 64
    assert norm.BN_CHUNK == _capi.VAMP_BN_CHUNK == header.constants["VAMP_BN_CHUNK"] == 4096
