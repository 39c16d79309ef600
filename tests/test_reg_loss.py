"""The masked regression losses on the device (ops.reg_losses / ops.reg_loss over
the HIP kernels of reg_loss.hip): packs of mean smooth-L1 / squared-error terms under a mask, without compaction.

Oracle (`oracle` below).  Loss: the fp32 element losses of torch-CPU (`reduction="none"`, which a CPU test pins bit
for bit to the stated formulas, |d| = 1 and d = 0 included) over a side, summed with math.fsum and divided in float64;
an empty side gives 0.  Gradient: upstream * l'(d) / |S_k| in float64 from the fp32 d.

Bounds, derived and not measured.  The kernels add the same fp32 element losses in float64: the accumulation error is
below n 2^-53 < 6e-10 relative for n < 2^22, far under half an fp32 ulp, so the loss is within ONE fp32 ulp of the
oracle rounded to fp32 (a flip at a rounding boundary is all that can happen).  The gradient is one float64 multiply
and one divide (combined relative error below 2.3e-16) before the single fp32 rounding: within ONE fp32 ulp of the
float64 formula rounded to fp32.  In addition the bar of tests/test_seg_loss.py holds for the loss and for every
grad_pred: with E_torch the error of the fp32 torch expression on compacted inputs (run eagerly on the same GPU)
against the float64 oracle, the HIP path's error may be at most max(2 E_torch, 1e-6); loss errors are relative,
gradient errors the largest absolute difference over the oracle gradient's largest magnitude.  Both errors are
printed.

Sizes are in units of T = ops.REG_TILE, the elements of one workgroup (a group of four elements per lane and round:
n = 1, 3 take the element path only, T - 1 ends in a partial group, T + 1 and 2T + 3 start a workgroup for 1 and 3
elements, 5T + 1 spans six workgroups)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, ops                           # noqa: E402
from vampire_amd.build import build_library                  # noqa: E402

T = ops.REG_TILE
SIZES = [1, 3, T - 1, T, T + 1, 2 * T + 3, 5 * T + 1]
KINDS = ("smooth_l1", "mse")
SIDES = ("set", "clear", "both")
UP = 1.7                                                     # the upstream gradient of the value tests


# ----------------------------------------------------------------------------- the oracle
def elem_np(kind, pred, target, dtype):
    """The stated element loss and its derivative in `dtype` arithmetic: (loss, l'(d))."""
    d = (np.asarray(pred, dtype=dtype) - np.asarray(target, dtype=dtype)).astype(dtype)
    if kind == "mse":
        return (d * d).astype(dtype), 2.0 * d.astype(np.float64)
    z = np.abs(d)
    half, one = dtype(0.5), dtype(1.0)
    with np.errstate(invalid="ignore"):
        loss = np.where(z < one, ((half * z).astype(dtype) * z).astype(dtype), (z - half).astype(dtype))
        lp = np.where(z < one, d.astype(np.float64), np.sign(d).astype(np.float64))
    return loss, lp


def elem_torch(kind, pred, target):
    """fp32 element losses of torch-CPU, reduction="none"."""
    fn = F.smooth_l1_loss if kind == "smooth_l1" else F.mse_loss
    return fn(pred.float().cpu(), target.float().cpu(), reduction="none")


def sides_of(side):
    return {"set": (True, False), "clear": (False, True), "both": (True, True)}[side]


def restate(kind, side, loss_elems, lp, mask, upstream=1.0):
    """The definition in float64 from element losses and derivatives: (loss, grad [n], (|S1|, |S0|))."""
    le, lp = np.asarray(loss_elems).reshape(-1), np.asarray(lp, dtype=np.float64).reshape(-1)
    m = np.ones(le.shape, bool) if mask is None else np.asarray(mask, dtype=bool).reshape(-1)
    loss, grad = 0.0, np.zeros(le.shape, np.float64)
    for sel, want in zip((m, ~m), sides_of(side)):
        cnt = int(sel.sum())
        if want and cnt:
            loss += math.fsum(le[sel].astype(np.float64).tolist()) / cnt
            grad[sel] = float(upstream) * lp[sel] / cnt
    return loss, grad, (int(m.sum()), int((~m).sum()))


def as_target(target, like):
    return target if torch.is_tensor(target) else torch.full(like.shape, float(target), dtype=torch.float32)


def oracle(kind, side, pred, target, mask, upstream=1.0):
    """pred (fp32 values; bf16 is widened), target (tensor or float), mask (bool tensor or None), all on the CPU."""
    p32 = pred.detach().float().cpu()
    t32 = as_target(target, p32)
    _, lp = elem_np(kind, p32.numpy().reshape(-1), t32.numpy().reshape(-1), np.float32)
    le = elem_torch(kind, p32, t32).numpy().reshape(-1)
    return restate(kind, side, le, lp, None if mask is None else mask.cpu().numpy(), float(np.float32(upstream)))


def host_expr(kind, a, b):
    """The training step's expressions on compacted inputs (multitask.MultiTaskLoss)."""
    return F.smooth_l1_loss(a, b) if kind == "smooth_l1" else ((a - b) ** 2).mean()


def torch_host(kind, side, pred, target, mask, upstream=1.0):
    """x[mask] / x[~mask] compaction + the host expression + autograd, in pred's dtype on pred's device."""
    x = pred.detach().clone().requires_grad_(True)
    t = as_target(target, pred).to(device=x.device, dtype=x.dtype)
    m = torch.ones(x.shape, dtype=torch.bool, device=x.device) if mask is None else mask.to(x.device)
    loss = x.sum() * 0.0
    for sel, want in zip((m, ~m), sides_of(side)):
        if want and bool(sel.any()):
            loss = loss + host_expr(kind, x[sel], t[sel])
    (loss * upstream).backward()
    return loss.detach(), x.grad


def make_case(n, seed=0, with_mask=True, const=False):
    g = torch.Generator().manual_seed(seed * 7919 + n)
    pred = 1.5 * torch.randn(n, generator=g)
    target = torch.randn(n, generator=g)
    mask = torch.rand(n, generator=g) >= 0.4
    mask[0] = True
    if n > 2:
        mask[1] = False
        target[:3] = torch.tensor([0.5, 0.25, 0.125])
        pred[:3] = torch.tensor([1.5, -0.75, 0.125])             # d = 1, -1, 0 exactly
    if const:
        target = 0.375
        if n > 2:
            pred[:3] = torch.tensor([1.375, -0.625, 0.375])
    return pred, target, (mask if with_mask else None)


def rel(a, ref):
    a, ref = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (a, ref))
    return abs(a - ref) / abs(ref) if ref != 0.0 else abs(a)


def gerr(a, ref):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    top = float(np.abs(ref).max())
    return float(np.abs(a.reshape(-1) - ref.reshape(-1)).max()) / (top if top > 0.0 else 1.0)


def within(name, e_hip, e_torch):
    print(f"  {name:34s} hip {e_hip:.3e}   torch fp32 {e_torch:.3e}")
    assert e_hip <= max(2 * e_torch, 1e-6), f"{name}: hip {e_hip:.3e} against torch {e_torch:.3e}"


def one_ulp(name, got, want64):
    """got (fp32) lies within one fp32 ulp of want64 rounded to fp32: it is that number or one of its neighbours."""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, dtype=np.float32).reshape(-1)
    w32 = np.asarray(want64, dtype=np.float64).reshape(-1).astype(np.float32)
    lo, hi = np.nextafter(w32, np.float32(-np.inf)), np.nextafter(w32, np.float32(np.inf))
    bad = ~((got >= lo) & (got <= hi))
    assert not bad.any(), f"{name}: {int(bad.sum())} of {got.size} beyond one ulp, first got {got[bad][0]!r} want {w32[bad][0]!r}"
    return int((got != w32).sum())


def run_hip(dev, pred, target, mask, kind, side, upstream=None):
    x = pred.to(dev).requires_grad_(True)
    t = target.to(dev) if torch.is_tensor(target) else target
    loss = ops.reg_loss(x, t, None if mask is None else mask.to(dev), kind, side)
    (loss if upstream is None else loss * upstream).backward()
    return loss.detach(), loss.counts, x.grad


# ----------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(T_=1, **kw):
    d = _capi.VampRegLossDesc()
    d.T = T_
    for t in range(max(T_, 0) if T_ <= 8 else 8):
        d.terms[t].n = 5000
    for k, v in kw.items():
        setattr(d.terms[0], k, v)
    return d


def _arrays(n_null=()):
    arrs = [(C.c_void_p * 8)(*[256 * (i + 1)] * 8) for i in range(4)]
    for a in n_null:
        arrs[a][0] = None
    return arrs


BAD = [(dict(T_=0), "T must be in [1, 8]"), (dict(T_=9), "T must be in [1, 8]"), (dict(n=0), "n must be in [1, 2^31)"),
       (dict(n=1 << 31), "n must be in [1, 2^31)"), (dict(kind=2), "kind must be"), (dict(side=3), "side must be"),
       (dict(side=-1), "side must be"), (dict(pred_dtype=_capi.VAMP_F16), "pred_dtype must be"),
       (dict(target_is_const=2), "target_is_const must be"), (dict(reserved=1), "reserved must be 0")]


@pytest.mark.parametrize("fields,message", BAD, ids=["T0", "T9", "n0", "n2^31", "kind", "side3", "side-1", "f16", "const2",
                                                     "reserved"])
def test_bad_descriptor_is_rejected_without_gpu(lib, fields, message):
    bad = _desc(**fields)
    pred, target, mask, grad = _arrays()
    out = [C.c_void_p(4096 * (i + 1)) for i in range(4)]
    assert lib.vamp_reg_loss_workspace_bytes(C.byref(bad)) == 0
    assert message in lib.vamp_last_error().decode()
    assert lib.vamp_reg_loss_forward(C.byref(bad), pred, target, mask, out[0], out[1], out[2], 1 << 40, None) == -1
    assert message in lib.vamp_last_error().decode()
    assert lib.vamp_reg_loss_backward(C.byref(bad), pred, target, mask, out[1], out[0], grad, None) == -1
    assert message in lib.vamp_last_error().decode()


def test_null_pointers_missing_mask_and_small_workspace_are_rejected(lib):
    """-1 before any launch: the fake addresses are never dereferenced."""
    d = _desc(T_=2)
    need = lib.vamp_reg_loss_workspace_bytes(C.byref(d))
    assert need >= 24 * 2 * 2                                    # two workgroups per term
    out = [C.c_void_p(4096 * (i + 1)) for i in range(4)]
    fwd = lambda a, lo=out[0], co=out[1], w=out[2], wb=need: lib.vamp_reg_loss_forward(C.byref(d), *a[:3], lo, co, w, wb, None)
    bwd = lambda a, co=out[1], gl=out[0]: lib.vamp_reg_loss_backward(C.byref(d), *a[:3], co, gl, a[3], None)
    assert fwd(_arrays(), wb=need - 1) == -1 and "workspace" in lib.vamp_last_error().decode()
    assert fwd(_arrays(), w=None) == -1
    assert fwd(_arrays(), lo=None) == -1 and fwd(_arrays(), co=None) == -1
    assert fwd(_arrays(n_null=(0,))) == -1 and "pred" in lib.vamp_last_error().decode()
    assert fwd(_arrays(n_null=(1,))) == -1 and "target" in lib.vamp_last_error().decode()
    assert fwd([None] + _arrays()[1:]) == -1 and fwd(_arrays()[:1] + [None] + _arrays()[2:]) == -1
    assert bwd(_arrays(n_null=(0,))) == -1 and bwd(_arrays(), co=None) == -1 and bwd(_arrays(), gl=None) == -1
    assert bwd(_arrays()[:3] + [None]) == -1
    for side in (_capi.VAMP_REG_CLEAR, _capi.VAMP_REG_BOTH):     # a mask-dependent side without a mask
        d.terms[0].side = side
        assert fwd(_arrays(n_null=(2,))) == -1 and "needs a mask" in lib.vamp_last_error().decode()
        assert bwd(_arrays(n_null=(2,))) == -1 and "needs a mask" in lib.vamp_last_error().decode()
    d.terms[0].side = _capi.VAMP_REG_SET
    d.terms[0].target_is_const = 1                               # the constant stands in for the target pointer
    assert fwd(_arrays(n_null=(1,)), wb=need - 1) == -1 and "workspace" in lib.vamp_last_error().decode()


def test_descriptor_layout(lib):
    assert C.sizeof(_capi.VampRegTerm) == 32 and C.sizeof(_capi.VampRegLossDesc) == 8 + 8 * 32
    assert [f[0] for f in _capi.VampRegTerm._fields_] == ["n", "kind", "side", "pred_dtype", "target_is_const",
                                                          "target_value", "reserved"]
    assert [f[0] for f in _capi.VampRegLossDesc._fields_] == ["T", "reserved", "terms"]
    assert _capi.ABI_VERSION == 16 and lib.vamp_abi_version() == 16
    assert (ops.REG_TILE, ops.REG_MAX_TERMS) == (_capi.VAMP_REG_TILE, _capi.VAMP_REG_MAX_TERMS) == (4096, 8)
    d = _desc()
    sizes = []
    for n in (T, T + 1, 40 * T):
        d.terms[0].n = n
        sizes.append(lib.vamp_reg_loss_workspace_bytes(C.byref(d)))
    assert sizes[0] > 0 and sizes[2] > sizes[0] and sizes[2] >= 24 * 40


def test_cpu_tensors_and_wrong_arguments_are_refused():
    x, y, m = torch.randn(10), torch.randn(10), torch.ones(10, dtype=torch.bool)
    with pytest.raises(_capi.VampireHipError):
        ops.reg_loss(x, y)
    with pytest.raises(_capi.VampireHipError):
        ops.reg_losses([ops.RegTerm(x, 0.5, m, "mse", "both")])
    with pytest.raises(ValueError):
        ops.reg_loss(x, y[:9])
    with pytest.raises(ValueError):
        ops.reg_loss(x, y, m[:9])
    with pytest.raises(ValueError):
        ops.reg_loss(x.reshape(2, 5), y)
    with pytest.raises(ValueError):
        ops.reg_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        ops.reg_loss(x, y, kind="l1")
    with pytest.raises(ValueError):
        ops.reg_loss(x, y, m, side="neither")
    with pytest.raises(ValueError):
        ops.reg_loss(x, y, None, side="both")                    # a mask-dependent side without a mask
    with pytest.raises(ValueError):
        ops.reg_loss(x[:0], y[:0])
    with pytest.raises(ValueError):
        ops.reg_losses([])
    with pytest.raises(ValueError):
        ops.reg_losses([ops.RegTerm(x, y)] * 9)
    with pytest.raises(TypeError):
        ops.reg_loss(torch.zeros(10, dtype=torch.long), y)
    assert ops.RegTerm(x, y) == (x, y, None, "smooth_l1", "set")


@pytest.mark.parametrize("kind", KINDS)
def test_element_formulas_are_torch_cpu_bit_for_bit(kind):
    """(0.5 z) z | z - 0.5 and d d in fp32 are what aten-CPU computes elementwise, |d| = 1 and d = 0 included."""
    g = torch.Generator().manual_seed(11)
    pred, target = 1.5 * torch.randn(20000, generator=g), torch.randn(20000, generator=g)
    target[:4] = torch.tensor([0.5, 0.25, 0.125, 3.0])
    pred[:4] = torch.tensor([1.5, -0.75, 0.125, 3.0 + 2.0 ** -20])
    mine, _ = elem_np(kind, pred.numpy(), target.numpy(), np.float32)
    theirs = elem_torch(kind, pred, target).numpy()
    assert mine.dtype == np.float32 and np.array_equal(mine.view(np.uint32), theirs.view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("side", SIDES)
def test_restatement_matches_float64_autograd(kind, side):
    """The definition (selection sets, float64 means, the gradient formula) in float64 numpy against float64 torch
    autograd of the host expressions on compacted inputs."""
    pred, target, mask = make_case(3001, seed=3)
    p64, t64 = pred.double(), target.double()
    le, lp = elem_np(kind, p64.numpy(), t64.numpy(), np.float64)
    loss, grad, counts = restate(kind, side, le, lp, mask.numpy(), upstream=UP)
    want, wg = torch_host(kind, side, p64, t64, mask, upstream=UP)
    e_loss, e_grad = rel(loss, want), gerr(grad, wg.numpy())
    print(f"\nrestatement {kind}/{side}: loss {e_loss:.2e}, gradient {e_grad:.2e}")
    assert e_loss <= 1e-13 and e_grad <= 1e-13
    assert counts == (int(mask.sum()), int((~mask).sum()))
    unsel = {"set": ~mask, "clear": mask, "both": torch.zeros_like(mask)}[side].numpy()
    assert bool((grad[unsel] == 0).all())
    # no mask is an all-true mask; an empty side contributes exactly 0
    a = restate(kind, "set", le, lp, None)
    b = restate(kind, "both", le, lp, np.ones(3001, bool))
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2] == (3001, 0)
    assert restate(kind, "clear", le, lp, np.ones(3001, bool))[0] == 0.0


# ----------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@gpu
@pytest.mark.parametrize("n", SIZES, ids=[f"n{n}" for n in SIZES])
def test_values_and_gradients(dev, n):
    """(a): both kinds, every side, with and without a mask, tensor and constant target, upstream gradient 1.7."""
    print(f"\nn = {n}")
    flips = 0
    for kind in KINDS:
        for const in (False, True):
            for with_mask, side in [(False, "set")] + [(True, s) for s in SIDES]:
                pred, target, mask = make_case(n, seed=1, with_mask=with_mask, const=const)
                name = f"{kind}/{side}/{'mask' if with_mask else 'all'}/{'const' if const else 'tensor'}"
                o_loss, o_grad, o_counts = oracle(kind, side, pred, target, mask, upstream=UP)
                loss, counts, grad = run_hip(dev, pred, target, mask, kind, side, upstream=UP)
                t_loss, t_grad = torch_host(kind, side, pred.to(dev), target, mask, upstream=UP)
                assert loss.dtype == torch.float32 and loss.dim() == 0 and grad.dtype == torch.float32
                assert counts.dtype == torch.int64 and tuple(counts.tolist()) == o_counts and not counts.requires_grad
                within(name + " loss", rel(loss, o_loss), rel(t_loss, o_loss))
                within(name + " grad_pred", gerr(grad, o_grad), gerr(t_grad, o_grad))
                flips += one_ulp(name + " loss", loss, o_loss)
                flips += one_ulp(name + " grad_pred", grad, o_grad)
                assert bool((grad.cpu().numpy()[o_grad == 0] == 0).all())
    print(f"  values one ulp off the rounded oracle: {flips}")


def pack_terms(dev, seed=2):
    """8 terms of sizes straddling tile edges, mixed kinds / sides / dtypes / targets."""
    spec = [(1, "mse", "set", None, torch.float32, True), (T - 1, "smooth_l1", "both", 1, torch.float32, False),
            (T, "mse", "clear", 1, torch.bfloat16, False), (T + 1, "smooth_l1", "set", 1, torch.bfloat16, True),
            (2 * T + 3, "mse", "both", 1, torch.float32, True), (3, "smooth_l1", "clear", 1, torch.float32, False),
            (5 * T + 1, "smooth_l1", "set", None, torch.float32, False), (T + 2, "mse", "both", 1, torch.bfloat16, False)]
    terms = []
    for k, (n, kind, side, m, dtype, const) in enumerate(spec):
        pred, target, mask = make_case(n, seed=seed + k, with_mask=m is not None, const=const)
        x = pred.to(dev).to(dtype).requires_grad_(True)
        t = target.to(dev) if torch.is_tensor(target) else target
        terms.append(ops.RegTerm(x, t, None if mask is None else mask.to(dev), kind, side))
    return terms


@gpu
def test_pack_is_bitwise_the_single_calls(dev):
    """(b)"""
    terms = pack_terms(dev)
    w = torch.linspace(0.5, 2.25, 8, device=dev)
    losses = ops.reg_losses(terms)
    assert losses.shape == (8,) and losses.dtype == torch.float32
    assert losses.counts.shape == (8, 2) and losses.counts.dtype == torch.int64 and not losses.counts.requires_grad
    (losses * w).sum().backward()
    pack_grads = [t.pred.grad.clone() for t in terms]
    for k, t in enumerate(terms):
        t.pred.grad = None
        one = ops.reg_loss(*t)
        (one * w[k]).backward()
        assert torch.equal(one.detach(), losses[k].detach()), k
        assert torch.equal(one.counts, losses.counts[k]), k
        assert t.pred.grad.dtype == t.pred.dtype and torch.equal(t.pred.grad, pack_grads[k]), k
        assert int(one.counts.sum()) == t.pred.numel()
    with pytest.raises(ValueError):
        ops.reg_losses(terms + terms[:1])
    # a term given as a plain tuple; a pred without requires_grad gets no gradient; none at all: no graph
    a, b = terms[1], terms[4]
    frozen = ops.RegTerm(b.pred.detach(), *b[1:])
    a.pred.grad = None
    two = ops.reg_losses([tuple(a), frozen])
    two.sum().backward()
    assert a.pred.grad is not None and torch.equal(two.detach(), losses[[1, 4]].detach())
    none = ops.reg_losses([frozen])
    assert none.grad_fn is None and not none.requires_grad and torch.equal(none, losses[[4]].detach())


@gpu
def test_terms_sharing_one_pred_accumulate(dev):
    """(b)"""
    pred, target, mask = make_case(2 * T + 3, seed=9)
    grads = []
    for kind, side in (("smooth_l1", "set"), ("mse", "clear")):
        grads.append(run_hip(dev, pred, target, mask, kind, side, upstream=UP)[2])
    x = pred.to(dev).requires_grad_(True)
    both = ops.reg_losses([ops.RegTerm(x, target.to(dev), mask.to(dev), "smooth_l1", "set"),
                           ops.RegTerm(x, target.to(dev), mask.to(dev), "mse", "clear")])
    (both.sum() * UP).backward()
    assert torch.equal(x.grad, grads[0] + grads[1])


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_alignment(dev, dtype):
    """(c): pred, target and mask as slices base[k : k + n], k in 0..3 independently per operand."""
    n = 2 * T + 3
    pred, target, mask = make_case(n, seed=4)
    pred = pred.to(dtype)
    w = torch.tensor([UP, 0.6], device=dev)

    def run(x, t, m):
        losses = ops.reg_losses([ops.RegTerm(x, t, m, "smooth_l1", "both"), ops.RegTerm(x, 0.375, m, "mse", "clear")])
        g, = torch.autograd.grad((losses * w).sum(), [x])
        return losses.detach(), losses.counts, g

    want = run(pred.to(dev).requires_grad_(True), target.to(dev), mask.to(dev))
    pad = lambda v, k: torch.cat([v.new_zeros(k), v, v.new_zeros(3 - k)]).to(dev)
    for kp in range(4):
        bp = pad(pred, kp).requires_grad_(True)
        for kt in range(4):
            bt = pad(target, kt)
            for km in range(4):
                bm = pad(mask, km)
                x, t, m = bp[kp: kp + n], bt[kt: kt + n], bm[km: km + n]
                assert x.data_ptr() % 16 == (kp * pred.element_size()) % 16 and m.data_ptr() % 4 == km
                got = run(x, t, m)
                assert all(torch.equal(a, b) for a, b in zip(got, want)), (kp, kt, km)


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_masked_out_poison(dev, kind):
    """(d): NaN / +-inf in pred and target outside the selected side reach neither the loss nor a gradient."""
    n = 2 * T + 3
    pred, target, mask = make_case(n, seed=5)
    poison = torch.tensor([float("nan"), float("inf"), float("-inf")]).repeat(n // 3 + 1)[:n]
    for side, out in (("set", ~mask), ("clear", mask)):
        for const in (False, True):
            t = 0.375 if const else target
            clean = run_hip(dev, pred, t, mask, kind, side, upstream=UP)
            bad_p = torch.where(out, poison, pred)
            bad_t = t if const else torch.where(out, poison.roll(1), target)
            got = run_hip(dev, bad_p, bad_t, mask, kind, side, upstream=UP)
            assert bool(torch.isfinite(got[0])) and all(torch.equal(a, b) for a, b in zip(got, clean)), (side, const)
            assert bool((got[2][out.to(dev)] == 0).all()) and int(out.sum()) > 0
    # `both` selects every element: the same poison does reach it (the select is not a blanket nan_to_num), and the
    # gradient at a selected NaN is NaN, as aten's backward gives it, at an infinity the sign (smooth-L1) or 2 d
    bad = torch.where(~mask, poison, pred)
    loss, _, grad = run_hip(dev, bad, target, mask, kind, "both")
    _, t_grad = torch_host(kind, "both", bad.to(dev), target, mask)
    assert not bool(torch.isfinite(loss))
    hit = torch.isnan(bad).to(dev)
    assert int(hit.sum()) > 0 and bool(torch.isnan(grad[hit]).all()) and bool(torch.isnan(t_grad[hit]).all())
    inf = torch.isinf(bad).to(dev)
    assert bool((torch.isnan(grad) == torch.isnan(t_grad)).all()) and torch.equal(grad[inf].sign(), t_grad[inf].sign())


@gpu
def test_edges(dev):
    """(e)"""
    n = 2 * T + 3
    pred, target, mask = make_case(n, seed=6)
    none, every = torch.zeros(n, dtype=torch.bool), torch.ones(n, dtype=torch.bool)
    for kind in KINDS:
        # an empty side: loss exactly 0, gradient all 0, no NaN
        for m, side in ((none, "set"), (every, "clear")):
            loss, counts, grad = run_hip(dev, pred, target, m, kind, side, upstream=UP)
            assert float(loss) == 0.0 and bool((grad == 0).all()) and 0 in counts.tolist() and n in counts.tolist()
        # `both` with one empty side is the other side alone
        for m, side in ((none, "clear"), (every, "set")):
            a, b = run_hip(dev, pred, target, m, kind, "both", upstream=UP), run_hip(dev, pred, target, m, kind, side, upstream=UP)
            assert all(torch.equal(x, y) for x, y in zip(a, b)) and float(a[0]) > 0
        # an all-true mask is no mask
        a, b = run_hip(dev, pred, target, every, kind, "set", upstream=UP), run_hip(dev, pred, target, None, kind, "set", upstream=UP)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        # both = set + clear.  With m1, m0 >= 0 the float64 means: both = fl(m1 + m0), set = fl(m1), clear = fl(m0), each
        # rounding within 2^-24 relative, so |both - (set + clear)| <= 2^-24 (m1 + m0 + m1 + m0) = 2^-23 (m1 + m0):
        # one fp32 rounding of the sum and one of each addend.  The gradients have disjoint supports: bitwise.
        s, c, bo = (run_hip(dev, pred, target, mask, kind, side, upstream=UP) for side in SIDES)
        total = float(s[0].double()) + float(c[0].double())
        assert abs(float(bo[0].double()) - total) <= 2.0 ** -23 * total * (1 + 2.0 ** -20)
        assert torch.equal(bo[2], s[2] + c[2]) and torch.equal(bo[1], s[1]) and torch.equal(bo[1], c[1])
        # a repeated call is bitwise equal
        again = run_hip(dev, pred, target, mask, kind, "both", upstream=UP)
        assert all(torch.equal(x, y) for x, y in zip(again, bo))
    # non-contiguous operands, fp16 / fp64 preds, a mask that is not bool, a float64 target
    x2 = torch.stack([pred, pred + 1.0], 1).to(dev)
    want = run_hip(dev, pred, target, mask, "smooth_l1", "both")
    strided = x2[:, 0].requires_grad_(True)
    assert not strided.is_contiguous()
    loss = ops.reg_loss(strided, target.double().to(dev), mask.to(torch.uint8).to(dev) * 3, "smooth_l1", "both")
    g, = torch.autograd.grad(loss, [strided])
    assert torch.equal(loss.detach(), want[0]) and torch.equal(g, want[2])
    x64 = pred.double().to(dev).requires_grad_(True)
    loss = ops.reg_loss(x64, target.to(dev), mask.to(dev), "smooth_l1", "both")
    g, = torch.autograd.grad(loss, [x64])
    assert torch.equal(loss.detach(), want[0]) and g.dtype == torch.float64 and torch.equal(g.float(), want[2])
    h = pred.half()
    a = ops.reg_loss(h.to(dev), target.to(dev), mask.to(dev), "mse", "both")
    b = ops.reg_loss(h.float().to(dev), target.to(dev), mask.to(dev), "mse", "both")
    assert torch.equal(a, b)
    # multi-dimensional operands are taken flat
    p3 = pred[:2 * T].reshape(2, T // 2, 2)
    a = ops.reg_loss(p3.to(dev), target[:2 * T].reshape(p3.shape).to(dev), mask[:2 * T].reshape(p3.shape).to(dev), "mse", "both")
    b = ops.reg_loss(pred[:2 * T].to(dev), target[:2 * T].to(dev), mask[:2 * T].to(dev), "mse", "both")
    assert torch.equal(a, b) and a.dim() == 0


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_bf16_pred_is_read_in_place(dev, kind):
    """(f): a bf16 pred gives bitwise the loss of pred.float(); its gradient is the fp32 call's .bfloat16()."""
    for n in (3, T + 1, 2 * T + 3):
        pred, target, mask = make_case(n, seed=7)
        h = pred.bfloat16()
        for side in SIDES:
            a = run_hip(dev, h, target, mask, kind, side, upstream=UP)
            b = run_hip(dev, h.float(), target, mask, kind, side, upstream=UP)
            assert a[2].dtype == torch.bfloat16 and b[2].dtype == torch.float32
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2].bfloat16()), (n, side)


@gpu
def test_no_sync_and_graph_replay(dev):
    """(g): a 3-term pack, n = 4T + 1, forward plus autograd.grad, with host synchronisation an error: eagerly, on a
    side stream and captured; replays after the inputs are overwritten in place are bitwise the eager results."""
    n = 4 * T + 1

    def inputs(seed):
        a, b, c = (make_case(n, seed=seed + k) for k in range(3))
        return [a[0], a[1], a[2], b[0].bfloat16(), b[2], c[0], c[1], c[2]]

    x0, t0, m0, x1, m1, x2, t2, m2 = (v.to(dev) for v in inputs(20))
    leaves = [x0.requires_grad_(True), x1.requires_grad_(True), x2.requires_grad_(True)]
    w = torch.tensor([1.0, UP, 0.25], device=dev)

    def step():
        losses = ops.reg_losses([ops.RegTerm(x0, t0, m0, "smooth_l1", "set"), ops.RegTerm(x1, -1.0, m1, "mse", "both"),
                                 ops.RegTerm(x2, t2, m2, "smooth_l1", "clear")])
        return (losses.detach(), losses.counts) + torch.autograd.grad((losses * w).sum(), leaves)

    step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = step()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, out))
    for seed in (30, 40):
        with torch.no_grad():
            for dst, src in zip((x0, t0, m0, x1, m1, x2, t2, m2), inputs(seed)):
                dst.copy_(src)
        g.replay()
        ref = step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ref, out)), seed
        assert not torch.equal(ref[0], eager[0])
