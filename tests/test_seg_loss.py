"""The segmentation loss on the device (ops.seg_loss / MultiTaskLoss(seg_loss="device") over the HIP kernels of
seg_loss.hip): cross-entropy + Lovasz-softmax ('present' classes) of logits under a mask, without compaction.

Oracle: `restate64` below, a float64 numpy restatement of the kernels' algebra (softmax, the masked sort key, the
Jaccard step in closed form from integer counts, the gradient formula) on the same fp32 logits.  A CPU test pins it
to float64 autograd of F.cross_entropy + multitask.lovasz_softmax on the compacted inputs.  It takes the permutation
it evaluates as an argument: any permutation that sorts the errors gives a valid subgradient, so a path is compared
with the oracle UNDER THAT PATH'S OWN permutation, which keeps rank swaps between precisions out of the comparison.

Tolerance, for every comparison of the HIP path with the oracle: E_torch is the error of an fp32 torch restatement
(multitask.lovasz_softmax's op sequence with a stable sort, F.cross_entropy, autograd; run eagerly on the same GPU on
the compacted inputs) against the oracle under its own permutation; the HIP path's error may be at most
max(2 E_torch, 1e-6).  The factor 2 allows for a different summation order, the floor is 16 fp32 ulps of quantities of
order 1.  The error of the loss and of both terms is relative; the error of the gradient is its largest absolute
difference over the oracle gradient's largest magnitude.  Every comparison prints both errors.

Inputs (make_case): logits 3 randn, labels from the first C - 2 classes (two classes absent), about 40 % masked out
at random (element 0 is always kept, so that the one-element case has a valid element).  For P > 100 also: rows 10-19
are copies of rows 30-39 with their labels and mask (bit-equal errors, decided by the element index); +200 on class 0
of rows 50-54 and on class 1 of rows 55-59, all labelled 0 and kept (p exactly 1 and 0: errors of exactly 0 and 1,
sign(0)); three labels set to C and, where the dtype allows, one to -1 (invalid, counted out), all under a true mask.

The sort tile is 2048 records and the row and scan blocks are smaller, so P = 70 001 crosses a workgroup boundary in
every multi-block phase (35 tiles; the histogram scan of 256 x 35 counters does not, by design: one workgroup)."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, losses, ops                   # noqa: E402
from vampire_amd import multitask as M                       # noqa: E402
from vampire_amd.build import build_library                  # noqa: E402
from vampire_amd.config import CFG_TINY                      # noqa: E402

SHAPES = [(1, 4), (63, 2), (300, 18), (4097, 18), (70001, 18), (5000, 32)]
IDS = [f"P{p}-C{c}" for p, c in SHAPES]


# ----------------------------------------------------------------------------- the oracle
def seq_sum(a):
    """Sequential sum (numpy's reduction is pairwise): adding zeros in between changes nothing."""
    return float(np.cumsum(np.asarray(a, dtype=np.float64))[-1]) if len(a) else 0.0


def restate64(logits, labels, valid, perms=None, keys="f32", w_ce=1.0, w_lv=1.0):
    """The kernels' algebra in float64.  logits [P, C] fp32, labels [P] integers, valid [P] bool (mask and label in
    range).  perms: per class the flat indices of the valid elements in sorted order; None sorts here, IN PLACE over
    all P elements with the masked key -- keys="f32": bits(fp32 err) + 1 for a valid element, 0 for the others;
    keys="f64": the float64 error, -1 for the others -- descending, stable (equal keys by ascending index).
    Returns dict(loss, ce, lv, grad [P, C], perms, n, present)."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    P, Cn = x.shape
    valid = np.asarray(valid, dtype=bool)
    z = x - x.max(1, keepdims=True)
    e = np.exp(z)
    s = e.sum(1, keepdims=True)
    p = e / s
    lab = np.where(valid, np.asarray(labels).astype(np.int64), 0)
    fg = np.zeros((P, Cn))
    fg[np.arange(P), lab] = 1.0
    fg[~valid] = 0.0
    d = fg - p
    err = np.abs(d)
    n = int(valid.sum())
    grad = np.zeros((P, Cn))
    if n == 0:
        return dict(loss=0.0, ce=0.0, lv=0.0, grad=grad, perms=[np.zeros(0, np.int64)] * Cn, n=0, present=0)
    ce_i = np.where(valid, -(z - np.log(s))[np.arange(P), lab], 0.0)
    ce = seq_sum(ce_i) / n
    present = [c for c in range(Cn) if fg[:, c].sum() > 0]
    gp = np.zeros((P, Cn))
    lv, out = 0.0, []
    for c in range(Cn):
        if perms is None:
            if keys == "f32":
                k = np.where(valid, err[:, c].astype(np.float32).view(np.uint32).astype(np.int64) + 1, 0)
            else:
                k = np.where(valid, err[:, c], -1.0)
            order = np.argsort(-k, kind="stable")[:n]
        else:
            order = np.asarray(perms[c], dtype=np.int64)
        out.append(order)
        f = fg[order, c]
        G = f.sum()
        if G == 0:
            continue
        cum = np.cumsum(f)
        k1 = np.arange(1, n + 1, dtype=np.float64)
        I, U = G - cum, G + k1 - cum
        delta = np.where(f > 0, 1.0 / U, I / np.maximum((U - 1.0) * U, 1.0))
        lv += seq_sum(err[order, c] * delta)
        gp[order, c] = -np.sign(d[order, c]) * delta
    lv /= len(present)
    gp /= len(present)
    grad = w_ce * (p - fg) / n + w_lv * p * (gp - (p * gp).sum(1, keepdims=True))
    grad[~valid] = 0.0
    return dict(loss=w_ce * ce + w_lv * lv, ce=ce, lv=lv, grad=grad, perms=out, n=n, present=len(present))


def lovasz_stable(probas, labels):
    """multitask.lovasz_softmax's op sequence with a stable sort; also returns the permutation [C, P]."""
    P, Cn = probas.shape
    fg = F.one_hot(labels, Cn).to(probas.dtype).t().contiguous()
    present = fg.sum(1) > 0
    err, perm = (fg - probas.t()).abs().sort(dim=1, descending=True, stable=True)
    fgs = fg.gather(1, perm)
    gts = fgs.sum(1, keepdim=True)
    inter = gts - fgs.cumsum(1)
    union = gts + (1 - fgs).cumsum(1)
    jac = 1.0 - inter / union
    jac = torch.cat([jac[:, :1], jac[:, 1:] - jac[:, :-1]], 1)
    per_class = (err * jac).sum(1)
    return (per_class * present).sum() / present.sum().clamp(min=1), perm


def torch_fp32(xc, yc, w_ce=1.0, w_lv=1.0):
    """The fp32 torch path on compacted inputs: (loss, ce, lv, grad, perm [C, n] over the compacted elements)."""
    x = xc.detach().clone().float().requires_grad_(True)
    ce = F.cross_entropy(x, yc)
    lv, perm = lovasz_stable(F.softmax(x, dim=1), yc)
    loss = w_ce * ce + w_lv * lv
    grad, = torch.autograd.grad(loss, x)
    return loss.detach(), ce.detach(), lv.detach(), grad, perm


def make_case(P, Cn, seed=0, label_dtype=torch.int64):
    g = torch.Generator().manual_seed(seed + 1000 * Cn + P)
    logits = 3.0 * torch.randn(P, Cn, generator=g)
    labels = torch.randint(0, max(Cn - 2, 1), (P,), generator=g)
    mask = torch.rand(P, generator=g) >= 0.4
    mask[0] = True
    if P > 100:
        logits[10:20], labels[10:20], mask[10:20] = logits[30:40], labels[30:40], mask[30:40]
        logits[50:55, 0] += 200.0
        logits[55:60, 1] += 200.0
        labels[50:60], mask[50:60] = 0, True
        labels[[70, 80, 90]], mask[[70, 80, 90]] = Cn, True
        if label_dtype != torch.uint8:
            labels[95], mask[95] = -1, True
    return logits.contiguous(), labels.to(label_dtype), mask


def valid_of(labels, mask, Cn):
    lab = labels.long()
    v = (lab >= 0) & (lab < Cn)
    return v if mask is None else v & mask.bool()


@functools.lru_cache(maxsize=None)
def case(P, Cn):
    logits, labels, mask = make_case(P, Cn)
    return logits, labels, mask, valid_of(labels, mask, Cn)


def rel(a, ref):
    a, ref = (float(v.detach()) if torch.is_tensor(v) else float(v) for v in (a, ref))
    return abs(a - ref) / abs(ref)


def gerr(a, ref):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    return float(np.abs(a - ref).max()) / float(np.abs(ref).max())


def within(name, e_hip, e_torch):
    print(f"  {name:24s} hip {e_hip:.3e}   torch fp32 {e_torch:.3e}")
    assert e_hip <= max(2 * e_torch, 1e-6), f"{name}: hip {e_hip:.3e} against torch {e_torch:.3e}"


def run_hip(logits, labels, mask, dev, scale=None, **kw):
    x = logits.to(dev).requires_grad_(True)
    loss = ops.seg_loss(x, labels.to(dev), None if mask is None else mask.to(dev), **kw)
    (loss if scale is None else loss * scale).backward()
    return loss.detach(), loss.terms, loss.n_valid, loss.n_present, x.grad


def window(logits, labels, mask, dev):
    """The device's sort: (n, present, sorted_err [C, P], perm [C, P]) on the CPU."""
    d, x, y, m = losses._seg_inputs(logits.to(dev), labels.to(dev), None if mask is None else mask.to(dev), 1.0, 1.0)
    _, _, counts, _, se, pm = losses._seg_forward(d, x, y, m, window=True)
    n, present = (int(v) for v in counts.cpu())
    return n, present, se.cpu(), pm.cpu().long()


@functools.lru_cache(maxsize=None)
def device_case(P, Cn):
    """The device's results for case(P, Cn), computed once: run_hip's tuple and the sort window."""
    dev = torch.device("cuda:0")
    logits, labels, mask, _ = case(P, Cn)
    return run_hip(logits, labels, mask, dev), window(logits, labels, mask, dev)


def compare(label, logits, labels, mask, dev, hip=None, win=None):
    """Loss, terms and gradient of the HIP path against the oracle under the device's permutation, the torch path
    against the oracle under its own; then the loss against the oracle with the oracle's own float64 sort."""
    Cn = logits.shape[1]
    valid = valid_of(labels, mask, Cn)
    loss, terms, n, present, grad = run_hip(logits, labels, mask, dev) if hip is None else hip
    wn, wp, _, perm = window(logits, labels, mask, dev) if win is None else win
    assert int(n) == wn == int(valid.sum()) and int(present) == wp
    o_dev = restate64(logits.numpy(), labels.numpy(), valid.numpy(), perms=[perm[c, :wn].numpy() for c in range(Cn)])
    vidx = valid.nonzero()[:, 0]
    t_loss, t_ce, t_lv, t_grad, t_perm = torch_fp32(logits[vidx].to(dev), labels[vidx].long().to(dev))
    o_t = restate64(logits.numpy(), labels.numpy(), valid.numpy(),
                    perms=[vidx[t_perm[c].cpu()].numpy() for c in range(Cn)])
    o_own = restate64(logits.numpy(), labels.numpy(), valid.numpy(), keys="f64")
    print(f"\n{label}: n = {wn}, present = {wp}")
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert terms.shape == (2,) and terms.dtype == torch.float32 and not terms.requires_grad
    within("loss", rel(loss, o_dev["loss"]), rel(t_loss, o_t["loss"]))
    within("term ce", rel(terms[0], o_dev["ce"]), rel(t_ce, o_t["ce"]))
    within("term lovasz", rel(terms[1], o_dev["lv"]), rel(t_lv, o_t["lv"]))
    tg = np.zeros_like(o_t["grad"])
    tg[vidx.numpy()] = t_grad.cpu().double().numpy()
    within("grad_logits", gerr(grad, o_dev["grad"]), gerr(tg, o_t["grad"]))
    within("loss, oracle's own sort", rel(loss, o_own["loss"]), rel(t_loss, o_own["loss"]))
    assert bool((grad.cpu()[~valid] == 0).all())
    return loss, terms, grad


# ----------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(**kw):
    d = _capi.VampSegLossDesc(1, 5000, 18, _capi.VAMP_SEG_ROWS, _capi.VAMP_I64, 0, 1.0, 1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD = [(dict(C=1), "C must be in [2, 32]"), (dict(C=33), "C must be in [2, 32]"),
       (dict(S=0), "B * S must be at least 1"), (dict(B=0), "B * S must be at least 1"),
       (dict(layout=2), "layout must be VAMP_SEG_ROWS or VAMP_SEG_PLANES"),
       (dict(S=1 << 27, C=16), "B * S * C must be below 2^31"), (dict(B=1 << 20, S=1 << 20, C=2), "below 2^31"),
       (dict(label_dtype=_capi.VAMP_F32), "label_dtype must be")]


@pytest.mark.parametrize("fields,message", BAD, ids=["C1", "C33", "S0", "B0", "layout", "2^31", "B*S", "labels"])
def test_bad_descriptor_is_rejected_without_gpu(lib, fields, message):
    bad = _desc(**fields)
    fake = [C.c_void_p(256 * (i + 1)) for i in range(10)]
    assert lib.vamp_seg_loss_workspace_bytes(C.byref(bad)) == 0
    assert message in lib.vamp_last_error().decode()
    assert lib.vamp_seg_loss_kept_bytes(C.byref(bad)) == 0
    assert lib.vamp_seg_loss_forward(C.byref(bad), *fake[:8], fake[8], 1 << 40, fake[9], 1 << 40, None) == -1
    assert message in lib.vamp_last_error().decode()
    assert lib.vamp_seg_loss_backward(C.byref(bad), *fake[:5], fake[8], 1 << 40, None) == -1
    assert message in lib.vamp_last_error().decode()


def test_null_pointers_and_small_buffers_are_rejected(lib):
    """VAMP_ENOSPC before any launch: the fake addresses are never dereferenced."""
    d = _desc()
    need, kept = lib.vamp_seg_loss_workspace_bytes(C.byref(d)), lib.vamp_seg_loss_kept_bytes(C.byref(d))
    assert need >= 16 * 18 * 5000 and kept >= 4 * 18 * 5000
    fake = [C.c_void_p(256 * (i + 1)) for i in range(10)]
    fwd = lambda a, k=fake[8], kb=kept, w=fake[9], wb=need: lib.vamp_seg_loss_forward(C.byref(d), *a, k, kb, w, wb, None)
    assert fwd(fake[:8], wb=need - 1) == -2
    assert "workspace" in lib.vamp_last_error().decode()
    assert fwd(fake[:8], kb=kept - 1) == -2
    assert "kept" in lib.vamp_last_error().decode()
    assert fwd(fake[:8], w=None) == -2 and fwd(fake[:8], k=None) == -2
    for hole in (0, 1, 3, 4, 5):                        # logits, labels, loss, terms, counts are required
        assert fwd([None if i == hole else fake[i] for i in range(8)]) == -2, hole
        assert "NULL" in lib.vamp_last_error().decode()
    bwd = lambda a, k=fake[8], kb=kept: lib.vamp_seg_loss_backward(C.byref(d), *a, k, kb, None)
    assert bwd(fake[:5], kb=kept - 1) == -2 and bwd(fake[:5], k=None) == -2
    for hole in (0, 1, 3, 4):                           # logits, labels, grad_loss, grad_logits
        assert bwd([None if i == hole else fake[i] for i in range(5)]) == -2, hole


def test_descriptor_layout(lib):
    assert C.sizeof(_capi.VampSegLossDesc) == 40
    assert [f[0] for f in _capi.VampSegLossDesc._fields_] == ["B", "S", "C", "layout", "label_dtype", "reserved",
                                                              "w_ce", "w_lv"]
    one, two = (lib.vamp_seg_loss_kept_bytes(C.byref(_desc(S=s))) for s in (5000, 10000))
    assert two > one


def test_cpu_tensors_and_wrong_shapes_are_refused():
    x, y = torch.randn(10, 6), torch.zeros(10, dtype=torch.long)
    with pytest.raises(_capi.VampireHipError):
        ops.seg_loss(x, y)
    with pytest.raises(_capi.VampireHipError):
        ops.seg_loss(x, y, torch.ones(10, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.seg_loss(x, y[:9])
    with pytest.raises(ValueError):
        ops.seg_loss(x, y, torch.ones(9, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.seg_loss(torch.randn(2, 5, 6), torch.zeros(5, 2, dtype=torch.long))
    with pytest.raises(ValueError):
        ops.seg_loss(torch.randn(10, 1), y)
    with pytest.raises(ValueError):
        ops.seg_loss(torch.randn(10, 33), y)
    with pytest.raises(TypeError):
        ops.seg_loss(x, y.float())
    head = M.BEVDepthHead(**M.reference_confs(CFG_TINY, output_channels=8, small_encoder=True)[1])
    with pytest.raises(ValueError):
        M.MultiTaskLoss(head, seg_loss="x")
    assert M.MultiTaskLoss(head).seg_loss == "host"
    assert M.MultiTaskLoss(head, seg_loss="device").seg_loss == "device"


def test_logit_layout_reads_channel_first_memory_in_place():
    from vampire_amd._tensors import _logit_layout
    occ = torch.randn(3, 6, 4, 5, 2).permute(0, 2, 3, 4, 1)
    cam = torch.randn(2, 3, 6, 4, 5).permute(0, 1, 3, 4, 2)
    bev = torch.randn(2, 6, 4, 5)[:, None, None].permute(0, 1, 2, 4, 5, 3)
    for x, B, S in ((occ, 3, 40), (cam, 6, 20), (bev, 2, 20)):
        layout, b, s, y = _logit_layout(x)
        assert (layout, b, s) == (_capi.VAMP_SEG_PLANES, B, S) and y is x
        flat = x.reshape(B * S, 6)
        mem = torch.as_strided(x, (B, 6, S), (6 * S, S, 1))
        assert torch.equal(flat, mem.permute(0, 2, 1).reshape(B * S, 6))
    rows = torch.randn(7, 6)
    assert _logit_layout(rows)[:3] == (_capi.VAMP_SEG_ROWS, 1, 7)
    assert _logit_layout(torch.randn(6, 7).t())[:3] == (_capi.VAMP_SEG_PLANES, 1, 7)
    odd = torch.randn(7, 12)[:, ::2]
    layout, b, s, y = _logit_layout(odd)
    assert (layout, b, s) == (_capi.VAMP_SEG_ROWS, 1, 7) and y.is_contiguous()


def test_restatement_matches_float64_autograd():
    """The closed-form Jaccard step, the masked key and the gradient formula against float64 autograd of
    F.cross_entropy + multitask.lovasz_softmax(softmax) on the compacted inputs; no ties in this input."""
    g = torch.Generator().manual_seed(3)
    P, Cn = 700, 7
    logits = 3.0 * torch.randn(P, Cn, generator=g)
    labels = torch.randint(0, Cn - 2, (P,), generator=g)
    mask = torch.rand(P, generator=g) >= 0.4
    labels[[5, 6]], mask[[5, 6]] = torch.tensor([Cn, -1]), True
    valid = valid_of(labels, mask, Cn)
    vidx = valid.nonzero()[:, 0]
    x = logits[vidx].double().requires_grad_(True)
    want = F.cross_entropy(x, labels[vidx]) + M.lovasz_softmax(F.softmax(x, dim=1), labels[vidx])
    wg, = torch.autograd.grad(want, x)
    got = restate64(logits.numpy(), labels.numpy(), valid.numpy(), keys="f64")
    top = float(wg.abs().max())
    eg = float(np.abs(got["grad"][vidx.numpy()] - wg.numpy()).max()) / top
    print(f"\nrestatement against float64 autograd: loss {rel(got['loss'], want):.2e}, gradient {eg:.2e}")
    assert rel(got["loss"], want) <= 1e-12 and eg <= 1e-12
    assert bool((got["grad"][~valid.numpy()] == 0).all())
    assert got["n"] == int(valid.sum()) and got["present"] == Cn - 2


def test_masked_key_in_place_equals_compaction():
    """Invalid elements given key 0 in place: exactly the loss (and the valid rows' gradient) of the compacted
    evaluation, ties included."""
    logits, labels, mask = make_case(3000, 18, seed=1)
    valid = valid_of(labels, mask, 18)
    vidx = valid.nonzero()[:, 0]
    a = restate64(logits.numpy(), labels.numpy(), valid.numpy())
    b = restate64(logits[vidx].numpy(), labels[vidx].numpy(), np.ones(len(vidx), bool))
    assert a["loss"] == b["loss"] and a["lv"] == b["lv"] and a["ce"] == b["ce"]
    assert np.array_equal(a["grad"][vidx.numpy()], b["grad"])
    for c in range(18):
        assert np.array_equal(a["perms"][c], vidx.numpy()[b["perms"][c]])


# ----------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@gpu
@pytest.mark.parametrize("P,Cn", SHAPES, ids=IDS)
def test_sort_is_exact(dev, P, Cn):
    """perm is the stable descending sort of the device's own keys over the valid elements, for every class."""
    logits, labels, mask, valid = case(P, Cn)
    (_, _, n_valid, n_present, _), (n, present, se, perm) = device_case(P, Cn)
    vidx = valid.nonzero()[:, 0]
    assert n == int(n_valid) == len(vidx)
    assert present == int(n_present) == len(torch.unique(labels.long()[vidx]))
    for c in range(Cn):
        assert torch.equal(perm[c, :n].sort().values, vidx), f"class {c}: not a permutation of the valid elements"
        back = torch.full((P,), float("nan"))
        back[perm[c, :n]] = se[c, :n]
        keys = back[vidx]
        assert bool(((keys >= 0) & (keys <= 1)).all())
        vals, order = torch.sort(keys, descending=True, stable=True)
        assert torch.equal(vals.view(torch.int32), se[c, :n].view(torch.int32)), f"class {c}: values"
        assert torch.equal(vidx[order], perm[c, :n]), f"class {c}: order"


@gpu
@pytest.mark.parametrize("P,Cn", SHAPES, ids=IDS)
def test_keys_are_the_errors(dev, P, Cn):
    logits, labels, mask, valid = case(P, Cn)
    _, (n, _, se, perm) = device_case(P, Cn)
    vidx = valid.nonzero()[:, 0]
    p = F.softmax(logits.double(), dim=1)
    fg = F.one_hot(labels.long().clamp(0, Cn - 1), Cn).double()
    want = (fg - p).abs()
    worst = 0.0
    for c in range(Cn):
        back = torch.zeros(P, dtype=torch.float64)
        back[perm[c, :n]] = se[c, :n].double()
        worst = max(worst, float((back[vidx] - want[vidx, c]).abs().max()))
    print(f"\nkeys P = {P}, C = {Cn}: largest |err - float64| = {worst:.3e}")
    assert worst <= 1e-6
    if P > 100:                                          # the saturated rows: errors of exactly 0 and exactly 1
        back = torch.zeros(P)
        back[perm[0, :n]] = se[0, :n]
        assert bool((back[50:55] == 0).all()) and bool((back[55:60] == 1).all())


@gpu
@pytest.mark.parametrize("P,Cn", SHAPES, ids=IDS)
def test_values_and_gradient(dev, P, Cn):
    logits, labels, mask, _ = case(P, Cn)
    hip, win = device_case(P, Cn)
    compare(f"P = {P}, C = {Cn}", logits, labels, mask, dev, hip, win)


@gpu
@pytest.mark.parametrize("dtype", [torch.int32, torch.uint8])
def test_label_dtypes(dev, dtype):
    logits, labels, mask = make_case(300, 18, label_dtype=dtype)
    a = run_hip(logits, labels, mask, dev)
    keep = valid_of(labels, mask, 18)
    b = run_hip(logits, labels.long(), keep, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@gpu
@pytest.mark.parametrize("name", ["small", "present_subset", "one_class", "single_pixel", "large"])
def test_reference_golden(dev, name):
    """The vectors of tests/golden/lovasz_golden.npz (the reference's lovasz_losses.py), with the tolerances
    test_lovasz_softmax_matches_reference_golden applies to the torch restatement."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "lovasz_golden.npz"))
    x, labels = torch.from_numpy(g[name + "_logits"]), torch.from_numpy(g[name + "_labels"])
    loss, terms, _, _, grad = run_hip(x, labels, None, dev, ce_weight=0.0, lovasz_weight=1.0)
    ref = torch.from_numpy(g[name + "_grad"])
    e = float((grad.cpu() - ref).abs().max())
    print(f"\ngolden {name}: loss {float(loss):.8f} (ref {float(g[name + '_loss']):.8f}), gradient error {e:.3e}, "
          f"bound {1e-7 + 2e-5 * float(ref.abs().max()):.3e}")
    assert float(loss) == pytest.approx(float(g[name + "_loss"]), rel=2e-6, abs=1e-7)
    assert float(terms[1]) == float(loss)
    assert e <= 1e-7 + 2e-5 * float(ref.abs().max())


@gpu
def test_layouts_and_mask_forms(dev):
    B, S, Cn = 3, 70, 18
    logits, labels, mask = make_case(B * S, Cn, seed=2)
    rows = run_hip(logits, labels, mask, dev)
    # the same numbers as channel-first memory [B, C, S] behind a permute view [B, S, C]
    mem = logits.reshape(B, S, Cn).permute(0, 2, 1).contiguous().to(dev)
    view = mem.permute(0, 2, 1).requires_grad_(True)
    assert not view.is_contiguous()
    loss = ops.seg_loss(view, labels.reshape(B, S).to(dev), mask.reshape(B, S).to(dev))
    loss.backward()
    assert torch.equal(loss.detach(), rows[0]) and torch.equal(loss.terms, rows[1])
    assert view.grad.shape == (B, S, Cn) and torch.equal(view.grad.reshape(B * S, Cn), rows[4])
    # no mask is an all-true mask
    a = run_hip(logits, labels, None, dev)
    b = run_hip(logits, labels, torch.ones(B * S, dtype=torch.bool), dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # a masked call is the unmasked call on the compacted rows
    valid = valid_of(labels, mask, Cn)
    comp = run_hip(logits[valid], labels[valid], None, dev)
    assert torch.equal(comp[0], rows[0]) and int(comp[2]) == int(rows[2]) and int(comp[3]) == int(rows[3])
    assert torch.equal(comp[4], rows[4][valid.to(dev)])
    assert bool((rows[4][~valid.to(dev)] == 0).all())


@gpu
def test_edges(dev):
    logits, labels, mask = make_case(300, 18, seed=4)
    # no valid element: everything exactly 0, no NaN
    loss, terms, n, present, grad = run_hip(logits, labels, torch.zeros(300, dtype=torch.bool), dev)
    assert float(loss) == 0.0 and terms.tolist() == [0.0, 0.0] and int(n) == 0 and int(present) == 0
    assert bool((grad == 0).all())
    # one valid element
    one = torch.zeros(300, dtype=torch.bool)
    one[123] = True
    compare("one valid element", logits, labels, one, dev)
    # every valid element of one class
    same = torch.full((300,), 3, dtype=torch.int64)
    compare("one class", logits, same, mask, dev)
    # repeatable, and the upstream gradient scales every element with one rounding
    a, b = run_hip(logits, labels, mask, dev), run_hip(logits, labels, mask, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    w1, w2 = window(logits, labels, mask, dev), window(logits, labels, mask, dev)
    assert w1[0] == w2[0] and all(torch.equal(w1[j][:, :w1[0]], w2[j][:, :w1[0]]) for j in (2, 3))
    s = run_hip(logits, labels, mask, dev, scale=3.0)
    want = 3.0 * a[4]
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, device=dev)) * 2.0 ** -23
    assert bool(((s[4] - want).abs() <= ulp).all()) and torch.equal(s[0], a[0])
    # no gradient wanted: the same loss, nothing to run backward
    loss = ops.seg_loss(logits.to(dev), labels.to(dev), mask.to(dev))
    assert torch.equal(loss.detach(), a[0]) and not loss.requires_grad and loss.grad_fn is None
    # bf16 logits are cast
    h = ops.seg_loss(logits.bfloat16().to(dev), labels.to(dev), mask.to(dev))
    f = ops.seg_loss(logits.bfloat16().float().to(dev), labels.to(dev), mask.to(dev))
    assert torch.equal(h, f)


@gpu
def test_no_sync_and_graph_replay(dev):
    P, Cn = 4097, 18
    logits, labels, mask = make_case(P, Cn, seed=5)
    x, y, m = logits.to(dev).requires_grad_(True), labels.to(dev), mask.to(dev)

    def step():
        loss = ops.seg_loss(x, y, m)
        return (loss.detach(), loss.terms, loss.n_valid, loss.n_present) + torch.autograd.grad(loss, [x])

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
    for seed in (6, 7):
        fl, fy, fm = make_case(P, Cn, seed=seed)
        with torch.no_grad():
            x.copy_(fl)
            y.copy_(fy)
            m.copy_(fm)
        g.replay()
        ref = step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ref, out)), seed
        assert not torch.equal(ref[0], eager[0])


@gpu
def test_multitask_seg_loss_on_the_device(dev, monkeypatch):
    cfg = dataclasses.replace(CFG_TINY, density_mode="sdf", final_dim=(192, 224), num_classes=6)
    torch.manual_seed(0)
    bb, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(cfg.sdf_bias)
    batch = M.synthetic_batch(cfg, 2, seed=5, device=dev, num_points=40, num_boxes=12)
    host_fn = M.MultiTaskLoss(model, sdf_bias=cfg.sdf_bias, det_targets="device", det_loss="device")
    dev_fn = M.MultiTaskLoss(model, sdf_bias=cfg.sdf_bias, det_targets="device", det_loss="device", seg_loss="device")
    assert host_fn.seg_loss == "host"
    sites, real = [], ops.seg_loss

    def recorder(logits, labels, mask=None, **kw):
        if logits.requires_grad:
            logits.retain_grad()
        sites.append((logits, labels, mask))
        return real(logits, labels, mask, **kw)

    monkeypatch.setattr(ops, "seg_loss", recorder)
    tg = dev_fn.targets(batch)
    out = model(batch[0], batch[1], inrange_pts=batch[11])
    with torch.no_grad():
        h_total = host_fn(out, batch, tg)
    d_total = dev_fn(out, batch, tg)
    d_total.backward()
    assert len(sites) == 4
    monkeypatch.setattr(ops, "seg_loss", real)
    print("\nMultiTaskLoss, tiny configuration")
    o_terms = []
    for name, (x, y, m) in zip(("camera", "bev", "lidar", "occupancy"), sites):
        Cn = x.shape[-1]
        flat = x.detach().float().reshape(-1, Cn).cpu()
        lab, msk = y.reshape(-1).cpu(), None if m is None else m.reshape(-1).cpu()
        valid = valid_of(lab, msk, Cn)
        assert int(valid.sum()) > 0, name
        n, _, _, perm = window(flat, lab, msk, dev)
        o_dev = restate64(flat.numpy(), lab.numpy(), valid.numpy(), perms=[perm[c, :n].numpy() for c in range(Cn)])
        vidx = valid.nonzero()[:, 0]
        t_loss, _, _, t_grad, t_perm = torch_fp32(flat[vidx].to(dev), lab[vidx].long().to(dev))
        o_t = restate64(flat.numpy(), lab.numpy(), valid.numpy(), perms=[vidx[t_perm[c].cpu()].numpy() for c in range(Cn)])
        tg64 = np.zeros_like(o_t["grad"])
        tg64[vidx.numpy()] = t_grad.cpu().double().numpy()
        within(f"{name} grad_logits", gerr(x.grad.reshape(-1, Cn), o_dev["grad"]), gerr(tg64, o_t["grad"]))
        o_terms.append(restate64(flat.numpy(), lab.numpy(), valid.numpy(), keys="f64")["loss"])
    hl, dl = host_fn.last, dev_fn.last
    for k in ("detection", "depth", "rgb", "sdf", "density", "camera_depth", "bev_height"):
        assert torch.equal(torch.as_tensor(hl[k]), torch.as_tensor(dl[k])), k
    o = dict(seg=o_terms[0] + o_terms[1], lidarseg=o_terms[2], occ=o_terms[3])
    for k in ("seg", "lidarseg", "occ"):
        within(f"last['{k}']", rel(dl[k], o[k]), rel(hl[k], o[k]))
    rest = float(h_total.double()) - sum(float(hl[k].double()) for k in ("seg", "lidarseg", "occ"))
    o_total = rest + sum(o.values())
    within("total", rel(d_total, o_total), rel(h_total, o_total))
    # the whole step with autocast: bf16 logits are cast, the permuted layouts are read in place
    loss = M.multitask_step(model, dev_fn, batch, amp_dtype=torch.bfloat16)
    assert torch.isfinite(loss) and all(torch.isfinite(torch.as_tensor(v)) for v in dev_fn.last.values())
