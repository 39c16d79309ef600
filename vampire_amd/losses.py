"""Training losses on plain tensors (Python over the C ABI).  All work happens in hand-written HIP kernels reached
through `_capi`; there is no CPU fallback."""
import collections
import ctypes as C

import torch

from . import _capi
from ._tensors import DTYPE_CODES, _logit_layout, _stream, as_labels, as_mask, need_device, refused

RGB_MIN_SIDE, RGB_MAX_CHANNELS, RGB_SCALES = 176, 4, 5
SEG_MIN_CLASSES, SEG_MAX_CLASSES = 2, 32
_SEG_LABEL_DTYPES = (torch.int64, torch.int32, torch.uint8)
REG_TILE, REG_MAX_TERMS = _capi.VAMP_REG_TILE, _capi.VAMP_REG_MAX_TERMS
_REG_KINDS = {"smooth_l1": _capi.VAMP_REG_SMOOTH_L1, "mse": _capi.VAMP_REG_MSE}
_REG_SIDES = {"set": _capi.VAMP_REG_SET, "clear": _capi.VAMP_REG_CLEAR, "both": _capi.VAMP_REG_BOTH}


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
        raise refused(vamp, "rgb_loss")
    need_device("rgb_loss", pred, target)
    loss, terms, vals = _RgbLoss.apply(d, pred.contiguous(), target.contiguous())
    loss.terms, loss.vals = terms, vals
    return loss


def _seg_forward(desc, logits, labels, mask, window=False):
    """One vamp_seg_loss_forward: (loss, terms, counts, kept, sorted_err, perm).  `window`: also export the sort --
    sorted_err [C, P] fp32 and perm [C, P] int32, a row's first counts[0] entries (the tests' view of the order)."""
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    terms = torch.empty(2, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    sorted_err = perm = None
    vamp = _capi.checked()
    with torch.cuda.device(dev):
        if window:
            sorted_err = torch.empty(desc.C, desc.B * desc.S, dtype=torch.float32, device=dev)
            perm = torch.empty(desc.C, desc.B * desc.S, dtype=torch.int32, device=dev)
        kept = torch.empty(vamp.vamp_seg_loss_kept_bytes(desc), dtype=torch.uint8, device=dev)
        ws = torch.empty(vamp.vamp_seg_loss_workspace_bytes(desc), dtype=torch.uint8, device=dev)
        vamp.vamp_seg_loss_forward(desc, logits, labels, mask, loss, terms, counts, sorted_err, perm, kept,
                                   kept.numel(), ws, ws.numel(), _stream())
    return loss, terms, counts, kept, sorted_err, perm


class _SegLoss(torch.autograd.Function):
    """loss, terms, counts = apply(desc, logits, labels, mask).  The forward's sort buffers are scratch of this call,
    handed back to the allocator on return; what the backward reads -- the unit gradients, 4 bytes per element and
    class, behind the two counts -- is a tensor of this call's own, kept in ctx."""

    @staticmethod
    def forward(ctx, desc, logits, labels, mask):
        loss, terms, counts, kept, _, _ = _seg_forward(desc, logits, labels, mask)
        ctx.desc = desc
        ctx.save_for_backward(logits, labels, mask, kept)
        ctx.mark_non_differentiable(terms, counts)
        return loss, terms, counts

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms, _grad_counts):
        logits, labels, mask, kept = ctx.saved_tensors
        grad = None
        if ctx.needs_input_grad[1]:
            grad = torch.empty_like(logits)              # (the logits' own strides: rows or channel-first planes)
            gl = grad_loss.to(torch.float32).contiguous()
            with torch.cuda.device(logits.device):
                _capi.checked().vamp_seg_loss_backward(ctx.desc, logits, labels, mask, gl, grad, kept, kept.numel(),
                                                       _stream())
        return None, grad, None, None


def _seg_inputs(logits, labels, mask, ce_weight, lovasz_weight, name="seg_loss"):
    """Checks and the descriptor of seg_loss: (desc, logits, labels, mask) as the entry points take them."""
    if logits.dim() < 1 or tuple(labels.shape) != tuple(logits.shape[:-1]):
        raise ValueError(f"{name}: labels {tuple(labels.shape)} do not match logits {tuple(logits.shape)}")
    if mask is not None and tuple(mask.shape) != tuple(labels.shape):
        raise ValueError(f"{name}: mask {tuple(mask.shape)} does not match labels {tuple(labels.shape)}")
    C = logits.shape[-1]
    if not SEG_MIN_CLASSES <= C <= SEG_MAX_CLASSES:
        raise ValueError(f"{name}: {C} classes are outside {SEG_MIN_CLASSES} <= C <= {SEG_MAX_CLASSES}")
    if labels.is_floating_point() or labels.requires_grad:
        raise TypeError(f"{name}: labels must be integers, got {labels.dtype}")
    need_device(name, logits, labels, mask)
    if logits.dtype != torch.float32:
        logits = logits.float()                          # (keeps a permuted view's channel-first memory)
    layout, B, S, logits = _logit_layout(logits)
    labels, mask = as_labels(labels, _SEG_LABEL_DTYPES), as_mask(mask)
    d = _capi.VampSegLossDesc(B, S, C, layout, DTYPE_CODES[labels.dtype], 0, float(ce_weight), float(lovasz_weight))
    vamp = _capi.checked()
    if vamp.vamp_seg_loss_workspace_bytes(d) == 0:
        raise refused(vamp, name)
    return d, logits, labels, mask


def seg_loss(logits, labels, mask=None, ce_weight=1.0, lovasz_weight=1.0):
    """The segmentation loss of base_exp.py:519-575 on the device (vamp_seg_loss_*): ce_weight * F.cross_entropy(x, y)
    + lovasz_weight * lovasz_softmax(F.softmax(x, 1), y) ('present' classes; multitask.lovasz_softmax) over x =
    logits[mask], y = labels[mask] -- without the boolean-mask compaction, so without a host synchronisation; no float
    atomics, bitwise repeatable, capturable in a graph.  logits [..., C], 2 <= C <= 32, read in place when contiguous
    or when they are the permute(.., 1)-style view of channel-first memory (the backbone's occ_logits, seg_p.permute(0,
    1, 3, 4, 2)); other dtypes than fp32 are cast.  labels (int64 | int32 | uint8, other integers cast) and mask (bool)
    are shaped like logits[..., 0].  Elements whose label lies outside [0, C) count as masked out.  Equal errors sort
    by ascending element index.  Returns the 0-dim fp32 loss; its attributes `terms` ([2]: CE, Lovasz), `n_valid` and
    `n_present` (0-dim int32) are detached device tensors.  The gradient goes to the logits only.  With no valid
    element the loss, both terms and the gradient are exactly 0 (F.cross_entropy of an empty selection is NaN)."""
    d, x, y, m = _seg_inputs(logits, labels, mask, ce_weight, lovasz_weight)
    loss, terms, counts = _SegLoss.apply(d, x, y, m)
    loss.terms, loss.n_valid, loss.n_present = terms, counts[0], counts[1]
    return loss


RegTerm = collections.namedtuple("RegTerm", ["pred", "target", "mask", "kind", "side"],
                                 defaults=(None, "smooth_l1", "set"))
RegTerm.__doc__ = """One term of ops.reg_losses: the mean `kind` ("smooth_l1", beta 1, or "mse") loss of `pred` against
`target` (a tensor shaped like pred, or a Python float) over the elements `mask` sets (side "set"), clears ("clear") or
the sum of both means ("both"); without a mask every element is set."""


def _ptr_array(tensors):
    return (C.c_void_p * REG_MAX_TERMS)(*[None if t is None else t.data_ptr() for t in tensors])


class _RegLosses(torch.autograd.Function):
    """losses, counts = apply(call, *preds); `call` = (desc, workspace bytes, targets, masks).  The forward's workspace
    is scratch of this call; the backward reads the operands again and `counts`.  The targets and masks are detached
    constants that are no inputs of the Function: they are kept on ctx as they are, next to the pointer arrays made
    from them; only the preds and `counts` go through save_for_backward."""

    @staticmethod
    def forward(ctx, call, *preds):
        desc, nbytes, targets, masks = call
        dev = preds[0].device
        ptrs = (_ptr_array(preds), _ptr_array(targets), _ptr_array(masks))
        with torch.cuda.device(dev):
            losses = torch.empty(desc.T, dtype=torch.float32, device=dev)
            counts = torch.empty(desc.T, 2, dtype=torch.int64, device=dev)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _capi.checked().vamp_reg_loss_forward(desc, *ptrs, losses, counts, ws, nbytes, _stream())
        ctx.desc, ctx.ptrs, ctx.constants = desc, ptrs, (targets, masks)
        ctx.save_for_backward(counts, *preds)
        ctx.mark_non_differentiable(counts)
        return losses, counts

    @staticmethod
    def backward(ctx, grad_losses, _grad_counts):
        counts, *preds = ctx.saved_tensors
        grads = [torch.empty_like(p) if ctx.needs_input_grad[1 + t] else None for t, p in enumerate(preds)]
        if any(g is not None for g in grads):
            gl = grad_losses.to(torch.float32).contiguous()
            with torch.cuda.device(counts.device):
                _capi.checked().vamp_reg_loss_backward(ctx.desc, *ctx.ptrs, counts, gl, _ptr_array(grads), _stream())
        return (None,) + tuple(grads)


def _reg_inputs(terms, name="reg_losses"):
    """Checks and the descriptor of reg_losses: ((desc, workspace bytes, targets, masks), preds) as _RegLosses and the
    entry points take them."""
    terms = [t if isinstance(t, RegTerm) else RegTerm(*t) for t in terms]
    if not 1 <= len(terms) <= REG_MAX_TERMS:
        raise ValueError(f"{name}: {len(terms)} terms are outside 1 <= T <= {REG_MAX_TERMS}")
    d = _capi.VampRegLossDesc()
    d.T = len(terms)
    preds, targets, masks = [], [], []
    for k, (pred, target, mask, kind, side) in enumerate(terms):
        if kind not in _REG_KINDS:
            raise ValueError(f"{name}: term {k}: kind must be one of {sorted(_REG_KINDS)}, got {kind!r}")
        if side not in _REG_SIDES:
            raise ValueError(f"{name}: term {k}: side must be one of {sorted(_REG_SIDES)}, got {side!r}")
        if not torch.is_tensor(pred) or not pred.is_floating_point():
            raise TypeError(f"{name}: term {k}: pred must be a floating-point tensor")
        const = not torch.is_tensor(target)
        if not const and tuple(target.shape) != tuple(pred.shape):
            raise ValueError(f"{name}: term {k}: target {tuple(target.shape)} does not match pred {tuple(pred.shape)}")
        if not const and target.requires_grad:
            raise ValueError(f"{name}: term {k}: there is no gradient with respect to target")
        if mask is not None and tuple(mask.shape) != tuple(pred.shape):
            raise ValueError(f"{name}: term {k}: mask {tuple(mask.shape)} does not match pred {tuple(pred.shape)}")
        if mask is None and side != "set":
            raise ValueError(f"{name}: term {k}: side {side!r} needs a mask")
        if pred.numel() < 1:
            raise ValueError(f"{name}: term {k}: pred is empty")
        need_device(name, pred, None if const else target, mask)
        if pred.dtype not in (torch.float32, torch.bfloat16):
            pred = pred.float()
        preds.append(pred.contiguous())
        targets.append(None if const else target.detach().to(torch.float32).contiguous())
        masks.append(as_mask(mask))
        m = d.terms[k]
        m.n, m.kind, m.side, m.pred_dtype = pred.numel(), _REG_KINDS[kind], _REG_SIDES[side], DTYPE_CODES[pred.dtype]
        m.target_is_const, m.target_value = int(const), float(target) if const else 0.0
    vamp = _capi.checked()
    nbytes = vamp.vamp_reg_loss_workspace_bytes(d)
    if nbytes == 0:
        raise refused(vamp, name)
    return (d, nbytes, targets, masks), preds


def reg_losses(terms):
    """The masked regression losses of base_exp.py:523-537 and :581-594 on the device (vamp_reg_loss_*): a pack of 1
    to 8 RegTerm evaluated in two launches, and the gradients of the whole pack in one, through autograd -- the mean
    smooth-L1 (beta 1) or squared error of pred against target over the elements the mask sets, clears, or the sum of
    both means, as F.smooth_l1_loss(pred[mask], target[mask]) and ((pred[mask] - target[mask]) ** 2).mean() give them,
    without the boolean-mask compaction, so without a host synchronisation; no atomics, bitwise repeatable, capturable
    in a graph.  pred is read in place when it is contiguous fp32 or bf16 (fp16 / fp64 are cast to fp32, other strides
    copied); target is cast to fp32; a mask that is not bool is taken as `!= 0`.  The one difference from the torch
    expressions: the mean over an empty selection is exactly 0, not NaN.  Returns the fp32 [T] losses; the attribute
    `counts` is the detached int64 [T, 2] tensor of (elements set, elements clear).  The gradient goes to the preds
    that require one (an element outside the selected side gets exactly 0), in pred's dtype; none goes to a target.
    The MultiTaskLoss of multitask.py does not use it yet."""
    call, preds = _reg_inputs(terms)
    losses, counts = _RegLosses.apply(call, *preds)
    losses.counts = counts
    return losses


def reg_loss(pred, target, mask=None, kind="smooth_l1", side="set"):
    """ops.reg_losses for one term: the 0-dim fp32 loss, `counts` int64 [2]."""
    call, preds = _reg_inputs([RegTerm(pred, target, mask, kind, side)], "reg_loss")
    losses, counts = _RegLosses.apply(call, *preds)
    loss = losses[0]
    loss.counts = counts[0]
    return loss
