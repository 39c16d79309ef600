"""Synchronised batch normalisation with the ReLU and the residual add that follow it, on the HIP kernels of
csrc/batch_norm.hip (vamp_bn_*).  The reference trains with `sync_batchnorm=True` (base_cli.py:78, 91):
every BatchNorm2d normalises over the batches of all ranks.  Four steps -- partial statistics, apply, and the same
two backward -- with one collective between the two of each direction; without a process group (or at world size 1)
the collective is a view and the module is a fused, bitwise repeatable, graph-capturable BatchNorm2d (+ ReLU, + add).

    norm = BatchNormAct2d(64, act="relu")            # parameters and buffers of nn.BatchNorm2d
    y = norm(conv(x), residual=identity)             # relu(bn(conv(x)) + identity), ONE autograd node

There is no fallback: a CPU tensor raises.  Everything is opt-in: `build_norm(None, c)` is today's nn.BatchNorm2d."""
import torch
import torch.distributed as dist
from torch import nn

from . import _capi
from ._tensors import DTYPE_CODES, FLOAT_DTYPES, _aligned, _stream, scratch

BN_CHUNK = _capi.VAMP_BN_CHUNK        # elements of one channel per workgroup: the split the tests' shapes are built on
MAX_WORLD = _capi.VAMP_BN_MAX_WORLD
_ACTS = {None: _capi.VAMP_BN_ACT_NONE, "relu": _capi.VAMP_BN_ACT_RELU}


def _act_code(act):
    if act not in _ACTS:
        raise ValueError(f"act must be None or 'relu', got {act!r}")
    return _ACTS[act]


def _operand(t, name, like=None):
    """A 4-D device tensor of a floating dtype as the kernels read it: NCHW-contiguous (a channels-last or otherwise
    strided tensor is copied: same values) and 16-byte aligned.  `like`: the tensor whose shape and dtype it must have."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _capi.VampireHipError(f"{name} must be a device tensor (no CPU fallback)")
    if like is None:
        if t.dim() != 4:
            raise ValueError(f"{name}: expected a 4-D [N, C, H, W] tensor, got shape {tuple(t.shape)}")
        if t.dtype not in FLOAT_DTYPES:
            raise TypeError(f"{name}: expected fp32, bf16 or fp16, got {t.dtype}")
    elif t.shape != like.shape or t.dtype != like.dtype:
        raise ValueError(f"{name}: expected shape {tuple(like.shape)} and dtype {like.dtype} (those of x), "
                         f"got {tuple(t.shape)} and {t.dtype}")
    return _aligned(t)


def _vector(t, name, C_, dtype=torch.float32):
    if not t.is_cuda:
        raise _capi.VampireHipError(f"{name} must be a device tensor (no CPU fallback)")
    if t.dtype != dtype or tuple(t.shape) != (C_,) or not t.is_contiguous():
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor of shape ({C_},), got {t.dtype} {tuple(t.shape)}")
    return t


def _rows(t, name, world, K):
    if not t.is_cuda:
        raise _capi.VampireHipError(f"{name} must be a device tensor (no CPU fallback)")
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != K:
        raise ValueError(f"{name}: expected float64 rows [world, {K}], got {t.dtype} {tuple(t.shape)}")
    if not 1 <= t.shape[0] <= MAX_WORLD:
        raise ValueError(f"{name}: {t.shape[0]} ranks, the kernels merge 1 .. {MAX_WORLD}")
    if world is not None and t.shape[0] != world:
        raise ValueError(f"{name}: expected {world} rows, got {t.shape[0]}")
    return t.contiguous()


def _desc(x, act=None, residual=False, training=True, world=1, eps=1e-5, momentum=0.1, update=False):
    d = _capi.VampBatchNormDesc()
    d.N, d.C, d.H, d.W = x.shape
    d.dtype, d.act, d.has_residual = DTYPE_CODES[x.dtype], _act_code(act), int(bool(residual))
    d.training, d.world, d.update_running = int(bool(training)), int(world), int(bool(update))
    d.eps, d.momentum = float(eps), float(momentum)
    return d


# =============================================================================================
# the four steps on plain tensors
# =============================================================================================
def bn_partial_stats(x):
    """This rank's float64 row [2 C + 1]: n = N H W, then per channel the mean and M2 = sum (x - mean)^2."""
    x = _operand(x, "x")
    vamp, d = _capi.checked(), _desc(x)
    row = torch.empty(2 * x.shape[1] + 1, dtype=torch.float64, device=x.device)
    ws = scratch("batch_norm", x.device, vamp.vamp_bn_workspace_bytes(d))
    vamp.vamp_bn_partial_stats(d, x, row, ws, ws.numel(), _stream())
    return row


def bn_apply(x, rows, weight, bias, eps=1e-5, act=None, residual=None, running_mean=None, running_var=None,
             momentum=0.1, num_batches_tracked=None):
    """y = act(weight (x - mean) invstd + bias [+ residual]) with the statistics of `rows` [world, 2 C + 1] (the ranks'
    rows in rank order).  Returns (y, saved): saved [3, C] fp32 holds mean, invstd and the low word of the float64 mean
    (what the backward steps take).  With running_mean and running_var they are updated in place (unbiased variance,
    global n); num_batches_tracked (int64) is incremented on the device."""
    x = _operand(x, "x")
    C_ = x.shape[1]
    rows = _rows(rows, "rows", None, 2 * C_ + 1)
    res = None if residual is None else _operand(residual, "residual", x)
    update = running_mean is not None
    if update != (running_var is not None):
        raise ValueError("running_mean and running_var come together")
    if update:
        _vector(running_mean, "running_mean", C_), _vector(running_var, "running_var", C_)
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1
                                            or not num_batches_tracked.is_cuda):
        raise ValueError("num_batches_tracked: expected one int64 element on the device")
    d = _desc(x, act, res is not None, True, rows.shape[0], eps, momentum, update)
    y = torch.empty_like(x)
    saved = torch.empty(3, C_, dtype=torch.float32, device=x.device)
    _capi.checked().vamp_bn_apply(d, x, res, rows, _vector(weight, "weight", C_), _vector(bias, "bias", C_),
                                  running_mean, running_var, num_batches_tracked, y, saved, _stream())
    return y, saved


def bn_apply_eval(x, weight, bias, running_mean, running_var, eps=1e-5, act=None, residual=None):
    """The apply kernel alone, with mean and 1 / sqrt(running_var + eps) from the running statistics."""
    x = _operand(x, "x")
    C_ = x.shape[1]
    res = None if residual is None else _operand(residual, "residual", x)
    d = _desc(x, act, res is not None, False, 1, eps, 0.0, False)
    y = torch.empty_like(x)
    _capi.checked().vamp_bn_apply(d, x, res, None, _vector(weight, "weight", C_), _vector(bias, "bias", C_),
                                  _vector(running_mean, "running_mean", C_), _vector(running_var, "running_var", C_),
                                  None, y, None, _stream())
    return y


def bn_backward_partial(dy, x, y, saved, act=None):
    """This rank's float64 row [2 C] (per channel sum dz and sum dz (x - mean)) and its grad_weight, grad_bias [C]
    fp32.  `y` is the saved output (read under act='relu' only: dz = dy where y > 0)."""
    x = _operand(x, "x")
    dy = _operand(dy, "dy", x)
    y = _operand(y, "y", x) if act is not None else None
    C_ = x.shape[1]
    vamp, d = _capi.checked(), _desc(x, act)
    row = torch.empty(2 * C_, dtype=torch.float64, device=x.device)
    gw, gb = torch.empty(C_, dtype=torch.float32, device=x.device), torch.empty(C_, dtype=torch.float32, device=x.device)
    ws = scratch("batch_norm", x.device, vamp.vamp_bn_workspace_bytes(d))
    vamp.vamp_bn_backward_partial(d, dy, x, y, _saved(saved, C_), row, gw, gb, ws, ws.numel(), _stream())
    return row, gw, gb


def bn_backward_apply(dy, x, y, saved, weight, rows, stat_rows, act=None, residual=False):
    """dx (and grad_residual = dz when `residual`) from the ranks' backward rows [world, 2 C] and the forward's rows
    [world, 2 C + 1] (for the global n), both in rank order."""
    x = _operand(x, "x")
    dy = _operand(dy, "dy", x)
    y = _operand(y, "y", x) if act is not None else None
    C_ = x.shape[1]
    stat_rows = _rows(stat_rows, "stat_rows", None, 2 * C_ + 1)
    rows = _rows(rows, "rows", stat_rows.shape[0], 2 * C_)
    d = _desc(x, act, residual, True, rows.shape[0])
    dx = torch.empty_like(x)
    gres = torch.empty_like(x) if residual else None
    _capi.checked().vamp_bn_backward_apply(d, dy, x, y, _saved(saved, C_), _vector(weight, "weight", C_), rows,
                                           stat_rows, dx, gres, _stream())
    return dx, gres


def _saved(saved, C_):
    if not saved.is_cuda or saved.dtype != torch.float32 or tuple(saved.shape) != (3, C_) or not saved.is_contiguous():
        raise ValueError(f"saved: expected the contiguous fp32 [3, {C_}] tensor bn_apply returned")
    return saved


def gather_rows(row, group=None):
    """[world, K]: the float64 row of every rank of `group`, in rank order, by one all_gather on the current stream.
    Without a group, or at world size 1, the [1, K] view of `row` itself."""
    if group is None or dist.get_world_size(group) == 1:
        return row.unsqueeze(0)
    world = dist.get_world_size(group)
    out = row.new_empty(world * row.numel())      # (the concatenated form: the one both gloo and RCCL take)
    dist.all_gather_into_tensor(out, row.contiguous(), group=group)
    return out.view(world, row.numel())


# =============================================================================================
# the module
# =============================================================================================
class _BatchNormActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, mod, group):
        ctx.in_dtype, ctx.act, ctx.has_res, ctx.group = x.dtype, mod.act, residual is not None, group
        ctx.training = mod.training
        x = _operand(x, "x")                      # (one contiguous copy at most, shared by the steps and the backward)
        residual = None if residual is None else _operand(residual, "residual", x)
        if not mod.training:
            return bn_apply_eval(x, weight, bias, mod.running_mean, mod.running_var, mod.eps, mod.act, residual)
        rows = gather_rows(bn_partial_stats(x), group)
        y, saved = bn_apply(x, rows, weight, bias, mod.eps, mod.act, residual, mod.running_mean, mod.running_var,
                            mod.momentum, mod.num_batches_tracked)
        # y only where the backward reads it (dz = dy where y > 0): a bare norm's output stays free for the in-place
        # ReLU that follows it in models built elsewhere, and the layer keeps one activation tensor less
        ctx.save_for_backward(x, y if mod.act is not None else None, saved, weight, rows)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        if not ctx.training:
            raise NotImplementedError("BatchNormAct2d: the backward in evaluation mode is not implemented (the reference "
                                      "trains with norm_eval=False); call .train() or run under torch.no_grad()")
        x, y, saved, weight, stat_rows = ctx.saved_tensors
        row, gw, gb = bn_backward_partial(dy, x, y, saved, ctx.act)
        dx = gres = None
        # (whether the second gather runs depends on the graph alone, which every rank shares: the collectives match)
        if ctx.needs_input_grad[0] or (ctx.has_res and ctx.needs_input_grad[1]):
            dx, gres = bn_backward_apply(dy, x, y, saved, weight, gather_rows(row, ctx.group), stat_rows, ctx.act,
                                         ctx.has_res)
        return dx, gres, gw, gb, None, None


class BatchNormAct2d(nn.BatchNorm2d):
    """nn.BatchNorm2d (same parameters, buffers and state dict) on the HIP kernels, with an optional fused ReLU
    (`act='relu'`) and residual (`forward(x, residual)`: act(bn(x) + residual)), synchronised over `process_group`
    (None: the default group when torch.distributed is initialised) whenever that group has more than one rank.
    One autograd node; saves x, y (under act='relu' only), mean / invstd and the gathered rows for the backward, no mask.  Evaluation mode
    normalises with the running statistics and has no backward."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, act=None,
                 process_group=None, device=None, dtype=None):
        if momentum is None:
            raise ValueError("BatchNormAct2d: momentum=None (a cumulative average) is not supported")
        if not affine:
            raise ValueError("BatchNormAct2d: affine=False is not supported")
        if not track_running_stats:
            raise ValueError("BatchNormAct2d: track_running_stats=False is not supported")
        super().__init__(num_features, eps, momentum, True, True, device=device, dtype=dtype)
        _act_code(act)
        self.act, self.process_group = act, process_group

    def extra_repr(self):
        return super().extra_repr() + f", act={self.act!r}"

    def _group(self):
        if not (dist.is_available() and dist.is_initialized()):
            return None
        group = self.process_group if self.process_group is not None else dist.group.WORLD
        return group if dist.get_world_size(group) > 1 else None

    def forward(self, x, residual=None):
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise _capi.VampireHipError("BatchNormAct2d: x must be a device tensor (no CPU fallback)")
        if x.dim() != 4:
            raise ValueError(f"BatchNormAct2d: expected a 4-D [N, C, H, W] input, got shape {tuple(x.shape)}")
        if x.shape[1] != self.num_features:
            raise ValueError(f"BatchNormAct2d: expected {self.num_features} channels, got {x.shape[1]}")
        if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype):
            raise ValueError(f"BatchNormAct2d: the residual must have x's shape and dtype ({tuple(x.shape)}, {x.dtype}), "
                             f"got {tuple(residual.shape)}, {residual.dtype}")
        group = self._group() if self.training else None
        if self.training and group is None and x.shape[0] * x.shape[2] * x.shape[3] == 1:
            raise ValueError("BatchNormAct2d: one value per channel (N H W == 1) has no variance to train with")
        return _BatchNormActFn.apply(x, residual, self.weight, self.bias, self, group)


def build_norm(norm_cfg, channels, act=None):
    """The 2-D norm layer of a `norm_cfg` (mmdet's names): None or dict(type='BN') -- nn.BatchNorm2d, `act` is the
    caller's to add; dict(type='SyncBN', eps=.., momentum=..) -- BatchNormAct2d carrying `act`."""
    cfg = dict(norm_cfg or dict(type="BN"))
    kind = cfg.pop("type", "BN")
    if kind == "BN":
        return nn.BatchNorm2d(channels, **cfg)
    if kind == "SyncBN":
        return BatchNormAct2d(channels, act=act, **cfg)
    raise ValueError(f"norm_cfg type must be 'BN' or 'SyncBN', got {kind!r}")


def is_fused(norm):
    """True for a norm layer that carries its own ReLU (and takes the residual in front of it): a BatchNormAct2d built
    with act='relu'.  One with act=None -- what convert_batch_norm makes -- is a plain norm, and its caller keeps its
    own activation."""
    return isinstance(norm, BatchNormAct2d) and norm.act == "relu"


def convert_batch_norm(module, process_group=None):
    """Every nn.BatchNorm2d of `module` replaced by a BatchNormAct2d(act=None) holding the SAME parameter and buffer
    tensors: synchronised statistics without the fusion, for a model built elsewhere.  Returns the module (a
    BatchNorm2d passed in directly is returned converted)."""
    if isinstance(module, nn.BatchNorm2d) and not isinstance(module, BatchNormAct2d):
        if module.momentum is None or not module.affine or not module.track_running_stats:
            raise ValueError("convert_batch_norm: momentum=None, affine=False and track_running_stats=False are not supported")
        new = BatchNormAct2d(module.num_features, module.eps, module.momentum, act=None, process_group=process_group,
                             device="meta")
        new.weight, new.bias = module.weight, module.bias
        for name in ("running_mean", "running_var", "num_batches_tracked"):
            new._buffers[name] = module._buffers[name]
        new.train(module.training)
        return new
    for name, child in module.named_children():
        converted = convert_batch_norm(child, process_group)
        if converted is not child:
            setattr(module, name, converted)
    return module
