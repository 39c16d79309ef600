"""The rgb loss on the device (ops.rgb_loss / MultiTaskLoss(rgb_loss="device") over the HIP kernels of rgb_loss.hip)
against a float64 CPU restatement (the oracle below: multitask.ms_ssim's definition plus F.smooth_l1_loss, gradients
by autograd) computed from the same fp32 inputs.

Tolerance, for every comparison of the HIP path with the oracle: E_torch is the error of the existing fp32 torch
expression of MultiTaskLoss (forward and autograd, run eagerly on the same GPU on the same inputs) against the same
oracle; the HIP path's error may be at most max(2 E_torch, 1e-6).  The factor 2 allows for a different summation
order, the floor is 16 fp32 ulps of quantities of order 1.  The error of the loss, of both terms and of each v[n, i]
is relative; the error of the gradient is its largest absolute difference over the oracle gradient's largest
magnitude.  Every comparison prints both errors.

Inputs: target = 0.5 + 0.25 sin(9 x + 5 y) over unit coordinates plus 0.15 rand, clamped to [0, 1]; pred = target +
0.2 randn; the label's top-left H/3 x W/3 block is the constant 0.25 (sigma_yy = 0 exactly) and pred is 0.25 on the
top-left H/4 x W/4 (both flat, sign(0) = 0); the first four pred elements are 2.5, -1.5, 1.0, 0.0 (the |d| > 1
branch of smooth-L1).  Every per-scale value stays above 0.1, so no image meets the relu rule except where a test
builds one that does."""
import ctypes as C
import dataclasses
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, ops                           # noqa: E402
from vampire_amd import multitask as M                       # noqa: E402
from vampire_amd.build import build_library                  # noqa: E402
from vampire_amd.config import CFG_TINY                      # noqa: E402

BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SHAPES = {"176x176": (1, 3, 176, 176), "179x203": (2, 1, 179, 203), "192x224": (3, 3, 192, 224)}


# ----------------------------------------------------------------------------- the oracle
def ms_ssim_vals(pred, target, data_range=1.0, k1=0.01, k2=0.03):
    """multitask.ms_ssim restated so that the per-image values are visible: (ms_ssim, v [N, 5])."""
    c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
    Cn = pred.shape[1]
    ax = torch.arange(11, device=pred.device, dtype=pred.dtype) - 5
    g = torch.exp(-(ax ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    win = (g[:, None] * g[None, :]).expand(Cn, 1, 11, 11).contiguous()
    conv = lambda t: F.conv2d(t, win, groups=Cn)
    vals, x, y = [], pred, target
    for i in range(5):
        mx, my = conv(x), conv(y)
        sxx, syy, sxy = conv(x * x) - mx * mx, conv(y * y) - my * my, conv(x * y) - mx * my
        v = (2 * sxy + c2) / (sxx + syy + c2)
        if i == 4:
            v = v * ((2 * mx * my + c1) / (mx ** 2 + my ** 2 + c1))
        vals.append(torch.relu(v.flatten(1).mean(1)))
        if i < 4:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    v = torch.stack(vals, 1)
    return torch.prod(v ** pred.new_tensor(BETAS)[None, :], 1).mean(), v


def oracle(pred, target, dtype=torch.float64):
    """(loss, terms [2], v [N, 5], grad_pred) in `dtype` on the inputs' device."""
    p = pred.detach().to(dtype).requires_grad_(True)
    t = target.detach().to(dtype)
    sl = F.smooth_l1_loss(p, t)
    ms, v = ms_ssim_vals(p, t)
    loss = sl + 1 - ms
    grad, = torch.autograd.grad(loss, p)
    return loss.detach(), torch.stack([sl, ms]).detach(), v.detach(), grad


def torch_expression(pred, target):
    """MultiTaskLoss's line, as it stands: (loss, grad_pred)."""
    p = pred.detach().clone().requires_grad_(True)
    loss = (F.smooth_l1_loss(p, target, reduction="none") + 1 - M.ms_ssim(p, target)).mean()
    grad, = torch.autograd.grad(loss, p)
    return loss.detach(), grad


def make_inputs(shape, seed=0, flat=True):
    N, Cn, H, W = shape
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.linspace(0, 1, H)[:, None], torch.linspace(0, 1, W)[None, :]
    target = ((0.5 + 0.25 * torch.sin(9 * xx + 5 * yy))[None, None] + 0.15 * torch.rand(N, Cn, H, W, generator=g))
    target = target.clamp(0, 1)
    pred = target + 0.2 * torch.randn(N, Cn, H, W, generator=g)
    if flat:
        target[..., :H // 3, :W // 3] = 0.25
        pred[..., :H // 4, :W // 4] = 0.25
    pred.view(-1)[:4] = torch.tensor([2.5, -1.5, 1.0, 0.0])
    return pred.contiguous(), target.contiguous()


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    pred, target = make_inputs(SHAPES[name], seed)
    return pred, target, oracle(pred, target)


def rel(a, ref):
    return abs(float(a) - float(ref)) / abs(float(ref))


def gerr(a, ref, top=None):
    """Largest absolute difference over the oracle's largest magnitude (`top`: a magnitude given by the caller)."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    top = float(ref.abs().max()) if top is None else top
    return float((a - ref).abs().max()) / top


def within(name, e_hip, e_torch):
    print(f"  {name:24s} hip {e_hip:.3e}   torch fp32 {e_torch:.3e}")
    assert e_hip <= max(2 * e_torch, 1e-6), f"{name}: hip {e_hip:.3e} against torch {e_torch:.3e}"


def run_hip(pred, target, dev, scale=None):
    p = pred.to(dev).requires_grad_(True)
    loss = ops.rgb_loss(p, target.to(dev))
    (loss if scale is None else loss * scale).backward()
    return loss.detach(), loss.terms, loss.vals, p.grad


def compare(label, pred, target, ora, dev, images=None, grad_top=None):
    """Loss, terms, v and the gradient of the HIP path and of the torch path against `ora`; `images`: the images whose
    gradient is compared (default all)."""
    o_loss, o_terms, o_v, o_grad = ora
    print(f"\n{label}")
    loss, terms, vals, grad = run_hip(pred, target, dev)
    pd, td = pred.to(dev), target.to(dev)
    t_loss, t_grad = torch_expression(pd, td)
    with torch.no_grad():
        t_ms, t_v = ms_ssim_vals(pd, td)
        t_terms = torch.stack([F.smooth_l1_loss(pd, td), t_ms])
    assert loss.dtype == torch.float32 and loss.dim() == 0
    assert terms.shape == (2,) and terms.dtype == torch.float32 and not terms.requires_grad
    assert vals.shape == o_v.shape and vals.dtype == torch.float32 and not vals.requires_grad
    within("loss", rel(loss, o_loss), rel(t_loss, o_loss))
    for j, name in enumerate(("smooth_l1", "ms_ssim")):
        within(f"term {name}", rel(terms[j], o_terms[j]), rel(t_terms[j], o_terms[j]))
    for n in range(o_v.shape[0]):
        for i in range(5):
            within(f"v[{n}, {i}]", rel(vals[n, i], o_v[n, i]), rel(t_v[n, i], o_v[n, i]))
    sel = slice(None) if images is None else images
    within("grad_pred", gerr(grad[sel], o_grad[sel], grad_top), gerr(t_grad[sel], o_grad[sel], grad_top))
    return loss, terms, vals, grad


# ----------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(**kw):
    d = _capi.VampRgbLossDesc(2, 3, 192, 224, 1.0, 0.01, 0.03)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_oracle_in_fp32_is_the_host_expression():
    """The oracle restates MultiTaskLoss's rgb line: evaluated in fp32 on the CPU it gives that loss to 1e-6, and
    no per-scale value of the test inputs comes near the relu."""
    for name in SHAPES:
        pred, target, ora = case(name)
        want, _ = torch_expression(pred, target)
        got = oracle(pred, target, dtype=torch.float32)[0]
        assert rel(got, want) <= 1e-6, (name, float(got), float(want))
        assert float(ora[2].min()) > 0.1, (name, ora[2])
        assert bool(torch.isfinite(ora[3]).all())


BAD = [(dict(N=0), "N must be positive"), (dict(C=0), "C must be in [1, 4]"), (dict(C=5), "C must be in [1, 4]"),
       (dict(H=175), "H, W must be at least 176"), (dict(W=175), "H, W must be at least 176")]


@pytest.mark.parametrize("fields,message", BAD, ids=["N0", "C0", "C5", "H175", "W175"])
def test_bad_descriptor_is_rejected_without_gpu(lib, fields, message):
    bad = _desc(**fields)
    fake = [C.c_void_p(256 * (i + 1)) for i in range(8)]
    assert lib.vamp_rgb_loss_workspace_bytes(C.byref(bad)) == 0
    assert message in lib.vamp_last_error().decode()
    assert lib.vamp_rgb_loss_forward(C.byref(bad), *fake[:5], fake[5], 1 << 40, None) == -1
    assert message in lib.vamp_last_error().decode()
    assert lib.vamp_rgb_loss_backward(C.byref(bad), *fake[:4], fake[5], 1 << 40, None) == -1
    assert message in lib.vamp_last_error().decode()


def test_null_pointers_and_small_workspace_are_rejected(lib):
    """VAMP_ENOSPC before any launch: the fake addresses are never dereferenced."""
    d = _desc()
    need = lib.vamp_rgb_loss_workspace_bytes(C.byref(d))
    assert need > 0
    fake = [C.c_void_p(256 * (i + 1)) for i in range(8)]
    assert lib.vamp_rgb_loss_forward(C.byref(d), *fake[:5], fake[5], need - 1, None) == -2
    assert "workspace" in lib.vamp_last_error().decode()
    assert lib.vamp_rgb_loss_forward(C.byref(d), *fake[:5], None, need, None) == -2
    for hole in range(5):
        args = [None if i == hole else fake[i] for i in range(5)]
        assert lib.vamp_rgb_loss_forward(C.byref(d), *args, fake[5], need, None) == -2, hole
    assert lib.vamp_rgb_loss_backward(C.byref(d), *fake[:4], fake[5], need - 1, None) == -2
    assert lib.vamp_rgb_loss_backward(C.byref(d), *fake[:4], None, need, None) == -2
    for hole in range(4):
        args = [None if i == hole else fake[i] for i in range(4)]
        assert lib.vamp_rgb_loss_backward(C.byref(d), *args, fake[5], need, None) == -2, hole


def test_descriptor_layout_and_workspace_size(lib):
    assert C.sizeof(_capi.VampRgbLossDesc) == 28
    assert [f[0] for f in _capi.VampRgbLossDesc._fields_] == ["N", "C", "H", "W", "data_range", "k1", "k2"]
    # the workspace grows with the batch, and holds at least the pooled images and three adjoint maps
    one, two = (lib.vamp_rgb_loss_workspace_bytes(C.byref(_desc(N=n))) for n in (1, 2))
    assert two > one >= 4 * 3 * (3 * 182 * 214 + 2 * 96 * 112)


def test_cpu_tensors_wrong_dtypes_and_shapes_are_refused():
    pred, target = torch.rand(1, 3, 176, 176), torch.rand(1, 3, 176, 176)
    with pytest.raises(_capi.VampireHipError):
        ops.rgb_loss(pred, target)
    with pytest.raises(TypeError):
        ops.rgb_loss(pred.bfloat16(), target)
    with pytest.raises(TypeError):
        ops.rgb_loss(pred, target.bfloat16())
    with pytest.raises(ValueError):
        ops.rgb_loss(torch.rand(1, 5, 176, 176), torch.rand(1, 5, 176, 176))
    with pytest.raises(ValueError):
        ops.rgb_loss(torch.rand(1, 3, 175, 176), torch.rand(1, 3, 175, 176))
    with pytest.raises(ValueError):
        ops.rgb_loss(pred, target[:, :2])
    with pytest.raises(ValueError):
        ops.rgb_loss(pred, target.clone().requires_grad_(True))
    head = M.BEVDepthHead(**M.reference_confs(CFG_TINY, output_channels=8, small_encoder=True)[1])
    with pytest.raises(ValueError):
        M.MultiTaskLoss(head, rgb_loss="x")
    assert M.MultiTaskLoss(head).rgb_loss == "host"


# ----------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_oracle(dev, shape):
    pred, target, ora = case(shape)
    compare(f"hand-built {shape} [N, C, H, W] = {SHAPES[shape]}", pred, target, ora, dev)


@gpu
def test_identical_images(dev):
    """pred = target: smooth-L1 is exactly 0 and ms_ssim is 1.  The oracle's gradient is zero up to float64 rounding
    here, so the rule's denominator is the largest magnitude of the oracle gradient of the ordinary prediction for
    the same label (the first shape's case): the scale a gradient of this loss has at this size."""
    pred, target, ora = case("176x176")
    same = target.clone()
    o = oracle(same, target)
    assert float(o[3].abs().max()) < 1e-12
    top = float(ora[3].abs().max())
    p = same.to(dev).requires_grad_(True)
    loss = ops.rgb_loss(p, target.to(dev))
    loss.backward()
    t_loss, t_grad = torch_expression(same.to(dev), target.to(dev))
    print(f"\nidentical images: terms {loss.terms.tolist()}  loss {float(loss):.3e}  torch loss {float(t_loss):.3e}")
    assert float(loss.terms[0]) == 0.0
    assert abs(float(loss.terms[1]) - 1.0) <= 1e-6
    assert bool(torch.isfinite(p.grad).all())
    within("grad_pred", gerr(p.grad, o[3], top), gerr(t_grad, o[3], top))


@gpu
def test_zero_scale_value(dev):
    """Image 0 is anti-correlated (pred = 1 - target on the textured label, no flat block): its first value is 0 after
    the relu, its MS-SSIM gradient is defined as 0 and only the smooth-L1 gradient is left.  Image 1 is ordinary."""
    shape = (2, 3, 176, 176)
    pred, target = make_inputs(shape, seed=3, flat=False)
    pred[0] = 1.0 - target[0]
    o_loss, o_terms, o_v, o_grad = oracle(pred, target)
    # whatever NaN the oracle (torch's definition: pow's backward at 0 is inf * 0) holds is confined to image 0; a
    # torch whose relu backward selects instead of multiplying drops it there too, so none is asked for
    assert bool(torch.isfinite(o_grad[1]).all())
    assert float(o_v[0, 0]) == 0.0 and float(o_v[1].min()) > 0.1
    loss, terms, vals, grad = run_hip(pred, target, dev)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(terms).all()) and bool(torch.isfinite(vals).all())
    assert bool(torch.isfinite(grad).all())
    assert float(vals[0, 0]) == 0.0
    print("\nzero scale value")
    within("loss", rel(loss, o_loss), rel(torch_expression(pred.to(dev), target.to(dev))[0], o_loss))
    # image 0: clamp(x - y, -1, 1) / numel, one rounding to fp32
    want = (pred[0].double() - target[0].double()).clamp(-1, 1) / pred.numel()
    got = grad[0].cpu().double()
    assert bool(((got - want).abs() <= want.abs() * 2.0 ** -23 + 2.0 ** -149).all())
    assert float(got.abs().max()) > 0
    # image 1 by the rule (the torch path is finite there as well)
    t_grad = torch_expression(pred.to(dev), target.to(dev))[1]
    assert bool(torch.isfinite(t_grad[1]).all())
    within("grad_pred, image 1", gerr(grad[1], o_grad[1]), gerr(t_grad[1], o_grad[1]))


@gpu
def test_exact_and_repeatable(dev):
    pred, target, _ = case("179x203")
    a, b = run_hip(pred, target, dev), run_hip(pred, target, dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the upstream gradient scales every element: one rounding each
    s = run_hip(pred, target, dev, scale=3.0)
    want = 3.0 * a[3]
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, device=dev)) * 2.0 ** -23
    assert bool(((s[3] - want).abs() <= ulp).all())
    assert torch.equal(s[0], a[0])
    # no gradient wanted: the same loss, nothing to run backward
    loss = ops.rgb_loss(pred.to(dev), target.to(dev))
    assert torch.equal(loss.detach(), a[0]) and not loss.requires_grad and loss.grad_fn is None
    assert torch.equal(loss.terms, a[1]) and torch.equal(loss.vals, a[2])


@gpu
def test_no_sync_and_graph_replay(dev):
    pred, target, _ = case("179x203")
    p, t = pred.to(dev).requires_grad_(True), target.to(dev)

    def step():
        loss = ops.rgb_loss(p, t)
        return (loss.detach(), loss.terms, loss.vals) + torch.autograd.grad(loss, [p])

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
        fp, ft = make_inputs(SHAPES["179x203"], seed)
        with torch.no_grad():
            p.copy_(fp)
            t.copy_(ft)
        g.replay()
        ref = step()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(ref, out)), seed
        assert not torch.equal(ref[0], eager[0])


@gpu
def test_multitask_rgb_loss_on_the_device(dev):
    cfg = dataclasses.replace(CFG_TINY, density_mode="sdf", final_dim=(192, 224), num_classes=6)
    torch.manual_seed(0)
    bb, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(cfg.sdf_bias)
    batch = M.synthetic_batch(cfg, 2, seed=5, device=dev, num_points=40, num_boxes=12)
    host_fn = M.MultiTaskLoss(model, sdf_bias=cfg.sdf_bias, det_targets="device", det_loss="device")
    dev_fn = M.MultiTaskLoss(model, sdf_bias=cfg.sdf_bias, det_targets="device", det_loss="device", rgb_loss="device")
    assert host_fn.rgb_loss == "host"
    tg = dev_fn.targets(batch)
    with torch.no_grad():
        out = model(batch[0], batch[1], inrange_pts=batch[11])
        host_fn(out, batch, tg)
        dev_fn(out, batch, tg)
        rgb_l = host_fn.downsampled_gt(batch[0][:, 0], batch[6][:, 0], batch[7][:, 0])[0]
    h, w = rgb_l.shape[-2:]
    assert (h, w) == (192, 224)
    rp, rl = out[1].float().reshape(-1, 3, h, w), rgb_l.reshape(-1, 3, h, w)
    o_loss = oracle(rp.cpu(), rl.cpu())[0]
    print("\nMultiTaskLoss, tiny configuration")
    hv, dv = host_fn.last["rgb"], dev_fn.last["rgb"]
    assert float(hv) > 0
    within("last['rgb']", rel(dv, o_loss), rel(hv, o_loss))
    loss = M.multitask_step(model, dev_fn, batch, amp_dtype=torch.bfloat16)
    assert torch.isfinite(loss) and torch.isfinite(dev_fn.last["rgb"])
    assert model.backbone.rgb_conv[0].weight.grad is not None
