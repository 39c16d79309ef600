"""The detection loss on the device (ops.det_loss / BEVDepthHead.loss_device over the HIP kernels of det_loss.hip)
against a float64 CPU restatement of the loss (the oracle below, gradients by autograd) computed from the same fp32
inputs.

Tolerance, for every comparison of the HIP path with the oracle: E_torch is the error of the existing fp32 torch
BEVDepthHead.loss (forward and autograd, run eagerly on the same GPU on the same inputs) against the same oracle;
the HIP path's error may be at most max(2 E_torch, 1e-6).  The error of a loss is relative; the error of a gradient
tensor is its largest absolute difference over the oracle tensor's largest magnitude.  The floor: every summed term
and both halves of each gradient expression have one sign, so a sum's error is bounded by the per-term error, and
1e-6 is about 16 fp32 ulps (the bar test_multitask_loss_with_device_targets already uses for this loss).  The
factor 2: the summation order differs and torch's own error depends on the input (saturated logits, where 1 - p
rounds in fp32, put 3e-6 into the loss of the smallest shape).  Every comparison prints both errors.  Each of the
[T, 2] terms is held to the same rule relative to its own oracle value, against the same term of the torch path
(torch_terms); a term whose oracle value is zero must be exactly zero.

With explicit counts, which the torch loss cannot take, E_torch is that of the torch loss with its own counts
against the oracle with the same: the factors scale loss and gradients and leave relative errors as they are.

Hand-built inputs: logits 3 randn - 2.19 with +20, -20, +100, -100 in front of each task and no logit within 1e-3
of +-ln 9999 (where the clamp switches the gradient off: one ulp of sigmoid decides there); heat = rand^8 with
about 0.5 % exact ones; random cells with slots 0, 1 and K - 1 sharing one and slots 2 and 3 another; masks about
60 % ones with those five live; one anno row with NaN in its last two columns, one equal to its prediction
(sign(0) = 0); code_weights [1] * 8 + [0.2, 0.2]."""
import ctypes as C
import dataclasses
import functools
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, ops                           # noqa: E402
from vampire_amd import multitask as M                       # noqa: E402
from vampire_amd.build import build_library                  # noqa: E402
from vampire_amd.config import CFG_A, CFG_TINY               # noqa: E402

KEYS = ("heatmap", "reg", "height", "dim", "rot", "vel")
CHANS = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2}
CW10 = [1.0] * 8 + [0.2, 0.2]
WB = 0.25
LN9999 = 9.21024
NCLS6 = tuple(t["num_class"] for t in M.TASKS)


# ----------------------------------------------------------------------------- the oracle
def oracle(preds, heats, anno, inds, masks, cw, wb, counts=None, dtype=torch.float64):
    """The loss of det_loss.hip's header restated with torch ops on the CPU in `dtype`.  preds: per task a dict of
    fp32 tensors; heats: per task [B, ncls, H, W]; anno [T, B, K, code], inds [T, B, K], masks [T, B, K].
    Returns (loss, terms [T, 2], grads: per task a dict like preds), all in `dtype`."""
    leaves = [{k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in p.items()} for p in preds]
    anno, inds, masks = anno.detach().cpu(), inds.detach().cpu(), masks.detach().cpu()
    cwt = torch.tensor(cw, dtype=dtype)
    terms = []
    for t, p in enumerate(leaves):
        h = heats[t].detach().cpu().to(dtype)
        s = torch.sigmoid(p["heatmap"])
        q = torch.clamp(s, min=1e-4, max=1 - 1e-4)
        pos = -(q + 1e-12).log() * (1 - q) ** 2 * (h == 1).to(dtype)
        neg = -(1 - q + 1e-12).log() * q ** 2 * (1 - h) ** 4
        n_pos = (h == 1).sum().to(dtype) if counts is None else counts[t, 0].detach().cpu().to(dtype)
        n_msk = masks[t].sum().to(dtype) if counts is None else counts[t, 1].detach().cpu().to(dtype)
        l_heat = (pos + neg).sum() / torch.clamp(n_pos, min=1)
        keys = [k for k in KEYS[1:] if k in p]
        box = torch.cat([p[k] for k in keys], 1)
        B, code = box.shape[:2]
        HW = box.shape[2] * box.shape[3]
        box = box.reshape(B, code, HW).permute(0, 2, 1)
        live = (masks[t] != 0) & (inds[t] >= 0) & (inds[t] < HW)
        got = box.gather(1, inds[t].clamp(0, HW - 1)[..., None].expand(-1, -1, code))
        tgt = anno[t].to(dtype)
        w = live[..., None].to(dtype) * (~tgt.isnan()).to(dtype) * cwt
        l_box = wb * ((got - torch.nan_to_num(tgt)).abs() * w).sum() / torch.clamp(n_msk, min=1e-4)
        terms.append(torch.stack([l_heat, l_box]))
    terms = torch.stack(terms)
    loss = terms.sum()
    flat = [v for p in leaves for v in p.values()]
    gflat = torch.autograd.grad(loss, flat)
    it = iter(gflat)
    grads = [{k: next(it) for k in p} for p in leaves]
    return loss.detach(), terms.detach(), grads


# ----------------------------------------------------------------------------- hand-built cases
@dataclasses.dataclass
class Case:
    preds: list          # per task {key: fp32 CPU tensor}
    heats: list          # per task [B, ncls, H, W] fp32
    anno: torch.Tensor
    inds: torch.Tensor
    masks: torch.Tensor
    cw: list
    ncls: tuple
    H: int
    W: int


@functools.lru_cache(maxsize=None)
def make_case(B, H, W, K, ncls, seed=0, vel=True, masks_zero=False, no_pos=False):
    g = torch.Generator().manual_seed(seed)
    T, HW, code = len(ncls), H * W, 10 if vel else 8
    preds, heats = [], []
    for n in ncls:
        x = 3 * torch.randn(B, n, H, W, generator=g) - 2.19
        x.view(-1)[:4] = torch.tensor([20.0, -20.0, 100.0, -100.0])
        x[((x - LN9999).abs() < 1e-3) | ((x + LN9999).abs() < 1e-3)] = 0
        p = {"heatmap": x}
        for k in KEYS[1:] if vel else KEYS[1:5]:
            p[k] = torch.randn(B, CHANS[k], H, W, generator=g)
        preds.append(p)
        h = torch.rand(B, n, H, W, generator=g) ** 8
        ones = torch.rand(B, n, H, W, generator=g) < 0.005
        if not no_pos:
            h[ones] = 1.0
            h.view(-1)[5] = 1.0
        assert no_pos == (int((h == 1).sum()) == 0)
        heats.append(h)
    inds = torch.randint(0, HW, (T, B, K), generator=g)
    inds[..., 1] = inds[..., 0]
    inds[..., K - 1] = inds[..., 0]
    inds[..., 2] = (inds[..., 0] + 1) % HW
    inds[..., 3] = inds[..., 2]
    masks = (torch.rand(T, B, K, generator=g) < 0.6).to(torch.uint8)
    masks[..., [0, 1, 2, 3, K - 1]] = 1
    masks[0, 0, 4] = 1
    if masks_zero:
        masks.zero_()
    anno = torch.randn(T, B, K, code, generator=g)
    anno[0, 0, 0, -2:] = float("nan")
    anno[0, 0, 4, 0] = preds[0]["reg"][0, 0].reshape(-1)[inds[0, 0, 4]]       # |pred - anno| = 0: sign(0) = 0
    return Case(preds, heats, anno, inds, masks, CW10[:code], tuple(ncls), H, W)


@functools.lru_cache(maxsize=None)
def case_oracle(*key, **kw):
    c = make_case(*key, **kw)
    return oracle(c.preds, c.heats, c.anno, c.inds, c.masks, c.cw, WB)


def to_dev(c, dev, detach=()):
    preds = [[{k: v.to(dev).requires_grad_(k not in detach) for k, v in p.items()}] for p in c.preds]
    tg = ops.DetTargets(torch.cat([h.reshape(-1) for h in c.heats]).to(dev), c.anno.to(dev), c.inds.to(dev),
                        c.masks.to(dev), c.ncls, c.H, c.W)
    return preds, tg


def run_hip(c, dev, counts=None, scale=None):
    preds, tg = to_dev(c, dev)
    loss = ops.det_loss(preds, tg, c.cw, WB, counts=counts)
    leaves = [v for pd in preds for v in pd[0].values()]
    g = torch.autograd.grad(loss if scale is None else scale * loss, leaves)
    it = iter(g)
    return loss.detach(), loss.terms, [{k: next(it) for k in pd[0]} for pd in preds]


def run_torch(c, dev):
    """The parent's path: BEVDepthHead.loss in fp32 on the GPU, eager, autograd to the predictions."""
    preds, tg = to_dev(c, dev)
    leaves = [dict(pd[0]) for pd in preds]
    stub = types.SimpleNamespace(train_cfg=dict(code_weights=c.cw), loss_bbox_weight=WB)
    loss = M.BEVDepthHead.loss(stub, tg.as_tuple(), preds)
    flat = [v for p in leaves for v in p.values()]
    g = torch.autograd.grad(loss, flat)
    it = iter(g)
    return loss.detach(), [{k: next(it) for k in p} for p in leaves]


def torch_terms(c, dev):
    """The (heat, box) terms as BEVDepthHead.loss computes them, fp32 on the GPU: its own clip_sigmoid and
    gaussian_focal_loss for the heatmap term, its lines restated for the box term (loss returns only their sum)."""
    preds, tg = to_dev(c, dev)
    heats, anno, inds, masks = tg.as_tuple()
    out = []
    with torch.no_grad():
        for t, pd in enumerate(preds):
            p = pd[0]
            heat = M.gaussian_focal_loss(M.clip_sigmoid(p["heatmap"]), heats[t],
                                         avg_factor=torch.clamp(heats[t].eq(1).float().sum(), min=1))
            box = torch.cat([p[k] for k in KEYS[1:] if k in p], dim=1)
            pred = box.permute(0, 2, 3, 1).reshape(box.shape[0], -1, box.shape[1])
            pred = pred.gather(1, inds[t][..., None].expand(-1, -1, pred.shape[2]))
            m = masks[t][..., None].expand_as(anno[t]).float() * (~torch.isnan(anno[t])).float()
            w = m * m.new_tensor(c.cw)
            num = torch.clamp(masks[t].float().sum(), min=1e-4)
            out.append(torch.stack([heat, WB * ((pred - torch.nan_to_num(anno[t])).abs() * w).sum() / num]))
    return torch.stack(out)


def rel(a, ref):
    return abs(float(a) - float(ref)) / abs(float(ref))


def gerr(a, ref):
    """Largest absolute difference over the oracle's largest magnitude; an all-zero oracle asks for exact zeros."""
    a, ref = a.detach().cpu().double(), ref.double()
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if float(a.abs().max()) == 0.0 else float("inf")
    return float((a - ref).abs().max()) / top


def within(name, e_hip, e_torch):
    print(f"  {name:28s} hip {e_hip:.3e}   torch fp32 {e_torch:.3e}")
    assert e_hip <= max(2 * e_torch, 1e-6), f"{name}: hip {e_hip:.3e} against torch {e_torch:.3e}"


def compare(label, c, dev, ora, ora_t=None, counts=None):
    """Loss, terms and every gradient of the HIP path against `ora`; the torch path against `ora_t` (its own
    counts), which is `ora` unless explicit counts were given."""
    o_loss, o_terms, o_grads = ora
    t_loss, _, t_grads_ref = ora_t or ora
    print(f"\n{label}")
    loss, terms, grads = run_hip(c, dev, counts=counts)
    th_loss, th_grads = run_torch(c, dev)
    e_t = rel(th_loss, t_loss)
    within("loss", rel(loss, o_loss), e_t)
    assert terms.shape == o_terms.shape and terms.dtype == torch.float32 and not terms.requires_grad
    # each term relative to its own oracle value, against the same term of the torch path; a zero term exactly
    th_terms, t_terms = torch_terms(c, dev), (ora_t or ora)[1]
    for t in range(o_terms.shape[0]):
        for j, name in enumerate(("heat", "box")):
            if float(o_terms[t, j]) == 0.0:
                assert float(terms[t, j]) == 0.0, f"term {name} of task {t} must be exactly 0"
            else:
                within(f"term task {t} {name}", rel(terms[t, j], o_terms[t, j]), rel(th_terms[t, j], t_terms[t, j]))
    for t, og in enumerate(o_grads):
        for k in og:
            within(f"grad task {t} {k}", gerr(grads[t][k], og[k]), gerr(th_grads[t][k], t_grads_ref[t][k]))
    return loss, terms, grads


# ----------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(**kw):
    d = _capi.VampDetLossDesc()
    d.B, d.T, d.H, d.W = 2, 6, 128, 128
    for t, n in enumerate(NCLS6):
        d.ncls[t] = n
    d.code, d.max_objs, d.has_vel = 10, 500, 1
    for c in range(10):
        d.code_weights[c] = CW10[c]
    d.loss_bbox_weight = WB
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_oracle_in_fp32_is_the_host_loss():
    """The oracle restates BEVDepthHead.loss: evaluated in fp32 on the CPU it gives the host loss to 1e-6."""
    torch.manual_seed(0)
    head = M.BEVDepthHead(**M.reference_confs(CFG_TINY, output_channels=8, small_encoder=True)[1])
    batch = M.synthetic_batch(CFG_TINY, 2, seed=3, num_points=10, num_boxes=12)
    heats, anno, inds, masks = head.get_targets(batch[4], batch[5])
    assert int(sum(m.sum() for m in masks)) > 0
    g = torch.Generator().manual_seed(1)
    B, _, H, W = heats[0].shape
    preds = []
    for h in heats:
        p = {"heatmap": 3 * torch.randn(h.shape, generator=g) - 2.19}
        for k in KEYS[1:]:
            p[k] = torch.randn(B, CHANS[k], H, W, generator=g)
        preds.append(p)
    cw = head.train_cfg["code_weights"]
    got, terms, _ = oracle(preds, heats, torch.stack(anno), torch.stack(inds), torch.stack(masks), cw,
                           head.loss_bbox_weight, dtype=torch.float32)
    ref = head.loss((heats, anno, inds, masks), [[{k: v.clone() for k, v in p.items()}] for p in preds])
    assert float(ref) > 0 and rel(got, ref) <= 1e-6
    assert got.dtype == torch.float32 and tuple(terms.shape) == (len(heats), 2)


BAD = [(dict(T=0), b"T must be in [1, 8]"), (dict(T=9), b"T must be in [1, 8]"), (dict(code=9), b"code must be 8 or 10"),
       (dict(code=10, has_vel=0), b"code must agree with has_vel"), (dict(H=0), b"H, W must be in")]


@pytest.mark.parametrize("fields,message", BAD, ids=["T0", "T9", "code9", "code10-novel", "H0"])
def test_bad_descriptor_is_rejected_without_gpu(lib, fields, message):
    ok = _desc()
    assert lib.vamp_det_loss_workspace_bytes(C.byref(ok)) > 0
    bad = _desc(**fields)
    fake = [C.c_void_p(256 * (i + 1)) for i in range(10)]
    assert lib.vamp_det_loss_workspace_bytes(C.byref(bad)) == 0
    assert message in lib.vamp_last_error(), lib.vamp_last_error()
    table = (_capi.VampDetTask * 8)()
    assert lib.vamp_det_loss_counts(C.byref(bad), fake[0], fake[1], fake[2], None) == -1
    assert message in lib.vamp_last_error(), lib.vamp_last_error()
    assert lib.vamp_det_loss_forward(C.byref(bad), table, *fake[:8], 1 << 30, None) == -1
    assert message in lib.vamp_last_error(), lib.vamp_last_error()
    assert lib.vamp_det_loss_backward(C.byref(bad), table, *fake[:6], table, fake[7], 1 << 30, None) == -1
    assert message in lib.vamp_last_error(), lib.vamp_last_error()


def test_null_pointers_and_small_workspace_are_rejected(lib):
    """VAMP_ENOSPC before any launch: the fake addresses are never dereferenced."""
    assert C.sizeof(_capi.VampDetLossDesc) == 112
    d = _desc()
    need = lib.vamp_det_loss_workspace_bytes(C.byref(d))
    assert need >= 8 * (d.T * d.B + 1)
    fake = [C.c_void_p(256 * (i + 1)) for i in range(10)]
    full = (_capi.VampDetTask * 6)(*[_capi.VampDetTask(*[4096 * (6 * t + j + 1) for j in range(6)]) for t in range(6)])
    holed = (_capi.VampDetTask * 6)(*[_capi.VampDetTask(*[4096 * (6 * t + j + 1) for j in range(6)]) for t in range(6)])
    holed[3].dim = None
    assert lib.vamp_det_loss_counts(C.byref(d), fake[0], None, fake[2], None) == -2
    assert lib.vamp_det_loss_counts(C.byref(d), fake[0], fake[1], None, None) == -2
    assert lib.vamp_det_loss_forward(C.byref(d), full, *fake[:7], fake[7], need - 1, None) == -2
    assert b"workspace" in lib.vamp_last_error()
    assert lib.vamp_det_loss_forward(C.byref(d), full, *fake[:7], None, need, None) == -2
    assert lib.vamp_det_loss_forward(C.byref(d), full, *fake[:5], None, fake[6], fake[7], need, None) == -2
    assert b"NULL" in lib.vamp_last_error()
    assert lib.vamp_det_loss_forward(C.byref(d), None, *fake[:7], fake[7], need, None) == -2
    assert lib.vamp_det_loss_forward(C.byref(d), holed, *fake[:7], fake[7], need, None) == -2
    assert b"task 3" in lib.vamp_last_error()
    assert lib.vamp_det_loss_backward(C.byref(d), full, *fake[:6], full, fake[7], need - 1, None) == -2
    assert b"workspace" in lib.vamp_last_error()
    assert lib.vamp_det_loss_backward(C.byref(d), full, *fake[:5], None, full, fake[7], need, None) == -2
    assert lib.vamp_det_loss_backward(C.byref(d), full, *fake[:6], None, fake[7], need, None) == -2
    assert lib.vamp_det_loss_backward(C.byref(d), holed, *fake[:6], full, fake[7], need, None) == -2


def test_cpu_tensors_wrong_dtypes_and_shapes_are_refused():
    c = make_case(3, 5, 7, 9, (1, 2, 3))
    cpu = lambda: [[dict(p)] for p in c.preds]
    tg = ops.DetTargets(torch.cat([h.reshape(-1) for h in c.heats]), c.anno, c.inds, c.masks, c.ncls, c.H, c.W)
    with pytest.raises(_capi.VampireHipError):
        ops.det_loss(cpu(), tg, c.cw)
    with pytest.raises(_capi.VampireHipError):
        ops.det_loss(cpu(), (c.heats, list(c.anno), list(c.inds), list(c.masks)), c.cw)
    with pytest.raises(TypeError):
        ops.det_loss([[{k: v.bfloat16() for k, v in p.items()}] for p in c.preds], tg, c.cw)
    head = M.BEVDepthHead(**M.reference_confs(CFG_TINY, output_channels=8, small_encoder=True)[1])
    with pytest.raises(_capi.VampireHipError):
        head.loss_device(tg, cpu())
    with pytest.raises(ValueError):
        M.MultiTaskLoss(head, det_loss="x")
    assert M.MultiTaskLoss(head).det_loss == "host"


# ----------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


SHAPES = {"5x7": (3, 5, 7, 9, (1, 2, 3)), "33x65": (2, 33, 65, 70, (1, 2)), "128x128": (2, 128, 128, 500, NCLS6)}


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_oracle(dev, shape):
    key = SHAPES[shape]
    compare(f"hand-built {shape} B={key[0]} K={key[3]} ncls={key[4]}", make_case(*key), dev, case_oracle(*key))


@gpu
@pytest.mark.parametrize("variant", ["no_vel", "T1", "T8", "masks_zero", "no_pos"])
def test_variants(dev, variant):
    key, kw = (3, 5, 7, 9, (1, 2, 3)), {}
    if variant == "no_vel":
        kw = dict(vel=False)
    elif variant == "T1":
        key = (3, 5, 7, 9, (2,))
    elif variant == "T8":
        key = (3, 5, 7, 9, (1, 2, 3, 4, 1, 2, 3, 4))
    elif variant == "masks_zero":
        kw = dict(masks_zero=True)
    elif variant == "no_pos":
        kw = dict(no_pos=True)
    c = make_case(*key, **kw)
    loss, terms, grads = compare(f"variant {variant}", c, dev, case_oracle(*key, **kw))
    if variant == "no_vel":
        assert all("vel" not in g for g in grads) and c.anno.shape[-1] == 8
    if variant == "masks_zero":
        assert bool((terms[:, 1] == 0).all())
        assert all(bool((v == 0).all()) for g in grads for k, v in g.items() if k != "heatmap")


@gpu
def test_explicit_counts(dev):
    key = (3, 5, 7, 9, (1, 2, 3))
    c = make_case(*key)
    true = torch.stack([torch.stack([(h == 1).sum().float(), m.sum().float()]) for h, m in zip(c.heats, c.masks)])
    for label, counts in (("half the true counts", true / 2), ("counts below the clamps", true * 0 + 1e-6)):
        ora = oracle(c.preds, c.heats, c.anno, c.inds, c.masks, c.cw, WB, counts=counts)
        compare(f"explicit counts: {label}", c, dev, ora, ora_t=case_oracle(*key), counts=counts.to(dev))
    preds, tg = to_dev(c, dev)
    with pytest.raises(ValueError):
        ops.det_loss(preds, tg, c.cw, counts=true[:2].to(dev))
    with pytest.raises(TypeError):
        ops.det_loss(preds, tg, c.cw, counts=true.double().to(dev))
    with pytest.raises(TypeError):
        ops.det_loss([[{k: v.bfloat16() for k, v in pd[0].items()}] for pd in preds], tg, c.cw)
    with pytest.raises(ValueError):
        ops.det_loss(preds[:2], tg, c.cw)
    with pytest.raises(ValueError):
        ops.det_loss(preds, tg, c.cw[:8])
    with pytest.raises(ValueError):                      # one task without vel among tasks with it
        ops.det_loss(preds[:2] + [[{k: v for k, v in preds[2][0].items() if k != "vel"}]], tg, c.cw)


@gpu
def test_masked_slot_with_an_index_outside_the_map_is_skipped(dev):
    """torch's gather asserts on such a slot; the kernels skip it without reading or writing through it."""
    key = (3, 5, 7, 9, (1, 2, 3))
    c = make_case(*key)
    counts = torch.tensor([[2.0, 7.0]] * 3, device=dev)
    bad = dataclasses.replace(c, inds=c.inds.clone())
    off = dataclasses.replace(c, masks=c.masks.clone())
    bad.inds[1, 2, 5], bad.inds[2, 0, 0] = 35, -1
    off.masks[1, 2, 5], off.masks[2, 0, 0] = 0, 0
    a, b = run_hip(bad, dev, counts=counts), run_hip(off, dev, counts=counts)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a[2], b[2]) for k in x)


def _cfg_a_case(dev):
    torch.manual_seed(0)
    head = M.BEVDepthHead(**M.reference_confs(CFG_A, output_channels=8, small_encoder=True)[1]).to(dev)
    batch = M.synthetic_batch(CFG_A, 2, seed=4, device=dev, num_points=10, num_boxes=12)
    tg = head.get_targets_device(batch[4], batch[5])
    x = torch.randn(2, 8, 128, 128, generator=torch.Generator().manual_seed(2)).to(dev)
    return head, tg, x


@gpu
def test_cfg_a_head(dev):
    head, tg, x = _cfg_a_case(dev)
    preds = head(x)
    w = head.shared_conv[0].weight
    ora = oracle([pd[0] for pd in preds], tg.heatmaps(), tg.anno, tg.inds, tg.masks, head.train_cfg["code_weights"],
                 head.loss_bbox_weight)
    o_loss, o_terms, o_grads = ora
    before = [dict(pd[0]) for pd in preds]
    dl = head.loss_device(tg, preds)
    assert all(list(pd[0]) == list(b) and all(pd[0][k] is b[k] for k in b)
               for pd, b in zip(preds, before)), "loss_device must leave the prediction dicts alone"
    hl = head.loss(tg.as_tuple(), [[{k: v.clone() for k, v in pd[0].items()}] for pd in preds])
    print("\ncfg-A head, B=2, 12 boxes")
    within("loss", rel(dl, o_loss), rel(hl, o_loss))
    flat = [v for pd in preds for v in pd[0].values()]
    w_ref, = torch.autograd.grad(flat, w, grad_outputs=[g.float().to(dev) for og in o_grads for g in og.values()],
                                 retain_graph=True)
    w_dev, = torch.autograd.grad(dl, w, retain_graph=True)
    w_host, = torch.autograd.grad(hl, w)
    within("grad shared_conv[0].weight", gerr(w_dev, w_ref.cpu()), gerr(w_host, w_ref.cpu()))


@gpu
def test_exact_and_repeatable(dev):
    key = SHAPES["33x65"]
    c = make_case(*key)
    a, b = run_hip(c, dev), run_hip(c, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a[2], b[2]) for k in x)
    # no live slot, no gradient: exactly zero
    HW = c.H * c.W
    for t, g in enumerate(a[2]):
        hit = torch.zeros(c.inds.shape[1], HW, dtype=torch.bool)
        for bi in range(c.inds.shape[1]):
            hit[bi, c.inds[t, bi][c.masks[t, bi] != 0]] = True
        for k in g:
            if k != "heatmap":
                v = g[k].cpu().reshape(g[k].shape[0], g[k].shape[1], HW)
                assert bool((v[~hit[:, None].expand_as(v)] == 0).all()), (t, k)
        assert float(g["reg"].abs().sum()) > 0
    # the upstream gradient scales every element: one rounding each
    s = run_hip(c, dev, scale=3.0)
    for x, y in zip(a[2], s[2]):
        for k in x:
            want = 3.0 * x[k]
            ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, device=dev)) * 2.0 ** -23
            assert bool(((y[k] - want).abs() <= ulp).all()), k
    # a detached heatmap: the box gradients as before, none for the heatmap
    preds, tg = to_dev(c, dev, detach=("heatmap",))
    held = [dict(pd[0]) for pd in preds]
    loss = ops.det_loss(preds, tg, c.cw, WB)
    loss.backward()
    assert torch.equal(loss.detach(), a[0])
    for t, pd in enumerate(preds):
        assert pd[0]["heatmap"].grad is None
        assert set(pd[0]) == set(held[t]) and all(pd[0][k] is held[t][k] for k in held[t])
        for k in pd[0]:
            if k != "heatmap":
                assert torch.equal(pd[0][k].grad, a[2][t][k]), (t, k)
    # get_targets's tuple of lists gives what the packed DetTargets gives
    preds, tg = to_dev(c, dev)
    assert torch.equal(ops.det_loss(preds, tg.as_tuple(), c.cw, WB).detach(), a[0])


@gpu
def test_no_sync_and_graph_replay(dev):
    key = SHAPES["33x65"]
    c = make_case(*key)
    preds, tg = to_dev(c, dev)
    leaves = [v for pd in preds for v in pd[0].values()]

    def step():
        loss = ops.det_loss(preds, tg, c.cw, WB)
        return (loss.detach(), loss.terms) + torch.autograd.grad(loss, leaves)

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
    assert all(torch.equal(x, y) for x, y in zip(eager, out))
    for seed in (5, 6, 7):
        f = make_case(*key, seed=seed)
        with torch.no_grad():
            for pd, p in zip(preds, f.preds):
                for k in p:
                    pd[0][k].copy_(p[k])
            tg.heat.copy_(torch.cat([h.reshape(-1) for h in f.heats]))
            tg.anno.copy_(f.anno)
            tg.inds.copy_(f.inds)
            tg.masks.copy_(f.masks)
        g.replay()
        ref = step()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(ref, out)), seed
        assert not torch.equal(ref[0], eager[0])


@gpu
def test_multitask_loss_on_the_device(dev):
    cfg = dataclasses.replace(CFG_TINY, density_mode="sdf", final_dim=(192, 224), num_classes=6)
    torch.manual_seed(0)
    bb, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(cfg.sdf_bias)
    batch = M.synthetic_batch(cfg, 2, seed=5, device=dev, num_points=40, num_boxes=12)
    host_fn = M.MultiTaskLoss(model, sdf_bias=cfg.sdf_bias, det_targets="device")
    dev_fn = M.MultiTaskLoss(model, sdf_bias=cfg.sdf_bias, det_targets="device", det_loss="device")
    tg = dev_fn.targets(batch)
    assert isinstance(tg, ops.DetTargets) and isinstance(host_fn.targets(batch), tuple)
    with torch.no_grad():
        out = model(batch[0], batch[1], inrange_pts=batch[11])
        fresh = lambda: [[{k: v.clone() for k, v in pd[0].items()}] for pd in out[0]]
        host_fn((fresh(),) + tuple(out[1:]), batch, host_fn.targets(batch))
        dev_fn(out, batch, tg)
    head = model.head
    o_loss = oracle([pd[0] for pd in out[0]], tg.heatmaps(), tg.anno, tg.inds, tg.masks,
                    head.train_cfg["code_weights"], head.loss_bbox_weight)[0]
    print("\nMultiTaskLoss, tiny configuration")
    h, d = host_fn.last["detection"], dev_fn.last["detection"]
    assert float(h) > 0
    within("last['detection']", rel(d, o_loss), rel(h, o_loss))
    loss = M.multitask_step(model, dev_fn, batch, amp_dtype=torch.bfloat16)
    assert torch.isfinite(loss) and torch.isfinite(dev_fn.last["detection"])
    assert model.head.shared_conv[0].weight.grad is not None
