"""Training losses on plain tensors (Python over the C ABI).  All work happens in hand-written HIP kernels reached
through `_capi`; there is no CPU fallback."""
import torch

from . import _capi
from ._tensors import _stream

RGB_MIN_SIDE, RGB_MAX_CHANNELS, RGB_SCALES = 176, 4, 5


class _RgbLoss(torch.autograd.Function):
    """loss, terms, vals = apply(desc, pred, target).  The forward's workspace (the pooled images, the per-pixel unit
    adjoints, the per-image factors) is what the backward reads, so it is a tensor of this call's own, kept in ctx;
    it is not allocated larger than the forward needs, and the caching allocator hands it back after the backward."""

    @staticmethod
    def forward(ctx, desc, pred, target):
        dev = pred.device
        loss = torch.empty((), dtype=torch.float32, device=dev)
        terms = torch.empty(2, dtype=torch.float32, device=dev)
        vals = torch.empty(desc.N, RGB_SCALES, dtype=torch.float32, device=dev)
        vamp = _capi.checked()
        with torch.cuda.device(dev):
            ws = torch.empty(vamp.vamp_rgb_loss_workspace_bytes(desc), dtype=torch.uint8, device=dev)
            vamp.vamp_rgb_loss_forward(desc, pred, target, loss, terms, vals, ws, ws.numel(), _stream())
        ctx.desc = desc
        ctx.save_for_backward(pred, target, ws)
        ctx.mark_non_differentiable(terms, vals)
        return loss, terms, vals

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms, _grad_vals):
        pred, target, ws = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[1]:
            grad = torch.empty_like(pred)
            gl = grad_loss.to(torch.float32).contiguous()
            with torch.cuda.device(pred.device):
                _capi.checked().vamp_rgb_loss_backward(ctx.desc, pred, target, gl, grad, ws, ws.numel(), _stream())
        return None, grad, None


def rgb_loss(pred, target, data_range=1.0):
    """The rgb loss of base_exp.py:539-549 on the device (vamp_rgb_loss_*): smooth_l1(pred, target).mean() + 1 -
    ms_ssim(pred, target), MS-SSIM with the defaults of multitask.ms_ssim, in six launches (five more for the gradient,
    through autograd), without a host synchronisation, without float atomics and bitwise repeatable; capturable in a
    graph.  pred, target: [N, C, H, W] fp32 device tensors (the caller casts), 1 <= C <= 4, H, W >= 176.  Returns the
    0-dim fp32 loss; its attributes `terms` ([2]: mean smooth-L1, ms_ssim) and `vals` ([N, 5]: the relu-ed per-image
    value of every scale) are detached fp32 tensors.  The gradient goes to pred only.  Where a scale's value of an
    image is 0 after the relu, the image's MS-SSIM gradient is exactly 0 (the torch expression yields NaN there)."""
    if pred.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"rgb_loss takes fp32 tensors, got {pred.dtype} and {target.dtype}")
    if target.requires_grad:
        raise ValueError("rgb_loss has no gradient with respect to target")
    if pred.dim() != 4 or pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} must be one [N, C, H, W] shape")
    N, C, H, W = pred.shape
    if N < 1 or not 1 <= C <= RGB_MAX_CHANNELS or H < RGB_MIN_SIDE or W < RGB_MIN_SIDE:
        raise ValueError(f"rgb_loss: [N, C, H, W] = {tuple(pred.shape)} is outside N >= 1, 1 <= C <= {RGB_MAX_CHANNELS}, "
                         f"H, W >= {RGB_MIN_SIDE}")
    d = _capi.VampRgbLossDesc(N, C, H, W, float(data_range), 0.01, 0.03)
    vamp = _capi.checked()
    if vamp.vamp_rgb_loss_workspace_bytes(d) == 0:
        raise ValueError(f"rgb_loss: {vamp.vamp_last_error().decode('utf-8', 'replace')}")
    if not (pred.is_cuda and target.is_cuda):
        raise _capi.VampireHipError("rgb_loss needs device tensors (no CPU fallback)")
    loss, terms, vals = _RgbLoss.apply(d, pred.contiguous(), target.contiguous())
    loss.terms, loss.vals = terms, vals
    return loss
