"""The parameter update that ends a training step, on the device (vamp_param_update_*, csrc/param_update.hip):
gradient clipping by the global norm, AdamW, the averaged (EMA) weights the reference evaluates and checkpoints with,
and the loss scale of fp16 training -- three launches per step whatever the number of tensors, no host
synchronisation, bitwise repeatable, capturable in a graph.  There is no fallback: CPU or non-fp32 parameters raise.

    upd = ParamUpdate(model, lr=2e-4)
    loss = multitask_step(model, loss_fn, batch, optimizer=upd)      # zero_grad(set_to_none=True) ... step()
    upd.copy_ema_to(eval_model)

The project's "plan on the host, then launch" pattern: `plan_update` is a pure function of the tensor sizes that lays
out the chunk table and the flat state; `ParamUpdate` fills in the addresses and launches."""
import collections
import typing

import numpy as np
import torch

from . import _capi
from ._tensors import _stream, refused

UPDATE_CHUNK = _capi.VAMP_UPDATE_CHUNK
KIND_PARAM, KIND_EMA_ONLY = _capi.VAMP_UPDATE_PARAM, _capi.VAMP_UPDATE_EMA_ONLY
STATE_ALIGN = 4                   # elements: a tensor's state starts on a 16-byte boundary
GROWTH_INTERVAL = _capi.VAMP_UPDATE_GROWTH_INTERVAL
INITIAL_SCALE = 65536.0

# the table in host memory, field for field VampUpdateChunk
CHUNK_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("state_off", "<i8"), ("len", "<i4"), ("kind", "<i4")])
# 32-bit word index of every field of VampUpdateScalars (64-bit fields: an even word)
_W = {"lr": 0, "step": 2, "updates": 4, "scale": 6, "growth": 7, "found_inf": 8, "total_norm": 9, "clip_coef": 10,
      "mult": 11, "decay_mul": 12, "step_size": 13, "bc2_sqrt": 14, "ema_d": 15, "ema_1md": 16}
_SCALAR_WORDS = 32


class UpdatePlan(typing.NamedTuple):
    """The layout `plan_update` returns.  Per chunk (numpy arrays of one length, parameter chunks first): `tensor` the
    index into `numels`, `offset` the chunk's first element in its tensor, `length`, `state_offset` its first element
    in the flat state, `kind`.  Per tensor: `tensor_state_offset`.  `param_state` elements of state cover every
    parameter (exp_avg, exp_avg_sq), `total_state` every tensor (ema)."""
    tensor: np.ndarray
    offset: np.ndarray
    length: np.ndarray
    state_offset: np.ndarray
    kind: np.ndarray
    tensor_state_offset: np.ndarray
    n_param_chunks: int
    n_buffer_chunks: int
    param_state: int
    total_state: int


def plan_update(numels, kinds, chunk=UPDATE_CHUNK) -> UpdatePlan:
    """Cut tensors of `numels` elements into chunks of at most `chunk` elements, a chunk never crossing a tensor, and
    lay their state out flat: tensors of kind KIND_PARAM first, then KIND_EMA_ONLY (buffers), each group in the given
    order, every tensor starting at a multiple of STATE_ALIGN elements.  A pure host function of its arguments."""
    numels = [int(n) for n in numels]
    kinds = [int(k) for k in kinds]
    if len(numels) != len(kinds):
        raise ValueError(f"{len(numels)} sizes but {len(kinds)} kinds")
    if chunk < STATE_ALIGN or chunk % STATE_ALIGN:
        raise ValueError(f"chunk must be a positive multiple of {STATE_ALIGN}, got {chunk}")
    if any(n < 0 for n in numels) or any(k not in (KIND_PARAM, KIND_EMA_ONLY) for k in kinds):
        raise ValueError("sizes must not be negative and kinds must be KIND_PARAM or KIND_EMA_ONLY")
    tensor, offset, length, state, kind = [], [], [], [], []
    tensor_state = np.zeros(len(numels), dtype=np.int64)
    counts, cursor, param_state = [0, 0], 0, 0
    for group in (KIND_PARAM, KIND_EMA_ONLY):
        for t, (n, k) in enumerate(zip(numels, kinds)):
            if k != group:
                continue
            tensor_state[t] = cursor
            for o in range(0, n, chunk):
                tensor.append(t)
                offset.append(o)
                length.append(min(chunk, n - o))
                state.append(cursor + o)
                kind.append(k)
                counts[group] += 1
            cursor += -(-n // STATE_ALIGN) * STATE_ALIGN
        if group == KIND_PARAM:
            param_state = cursor
    i64 = lambda v: np.asarray(v, dtype=np.int64)
    return UpdatePlan(i64(tensor), i64(offset), i64(length), i64(state), np.asarray(kind, dtype=np.int32), tensor_state,
                      counts[0], counts[1], param_state, cursor)


class ParamUpdate:
    """Clip + AdamW + EMA (+ loss scale) for every parameter and floating-point buffer of `model`, in place of a
    torch.optim.AdamW, a clip_grad_norm_ and the reference's EMA callback.

    lr, betas, eps, weight_decay: AdamW (decoupled decay), as torch.optim.AdamW computes a step.  max_norm: gradients
    are scaled by min(1, max_norm / (total_norm + 1e-6)); <= 0 or None: no clipping, the norm is still computed.
    ema_decay: the averaged weights e = e d + (1 - d) x of every floating-point state_dict entry, d = ema_decay (1 -
    exp(-n / 2000)) at update n (counted from `ema_updates`), initialised from the model; <= 0 or None: none are kept.
    loss_scale: None -- gradients are taken as they are; a float S -- they carry the factor S (see scale_loss), which
    the update divides out; "dynamic" -- S starts at 65536, halves on a step whose gradients hold an inf or NaN and
    doubles after 2000 steps without one (torch.amp.GradScaler's rule).  In every mode a step with a non-finite
    gradient leaves the parameters and the moments as they are (`stats["found_inf"]`); the EMA still moves.

    The parameters and buffers must keep their storage for the updater's life.  A gradient may move: step() compares
    every `p.grad.data_ptr()` with the chunk table and uploads a new table when one changed; a parameter without a
    gradient is left out of the norm and keeps its p, m and v on that step, as torch skips it (its EMA still moves).
    In a multi-GPU step, call step() after the gradients are averaged (GradSync.finish()): the average carries one
    rank's inf to every rank, so no collective is needed.

    One difference from torch.optim.AdamW: the step count t of the bias corrections 1 - beta^t is ONE counter for all
    parameters (stats["step"]: the steps without an overflow), where torch keeps one per parameter that counts the
    gradients that parameter has had.  The two agree for a parameter that has a gradient on every step, and for one
    that never has one (the reference's lidar-seg head with lidar_seg=False); they differ for a parameter whose
    gradient is missing on some steps and present on a later one.  Where a gradient first appears at global step 3
    with the default betas, torch moves the parameter by lr sign(g) and this update by ((1 - beta1) / (1 - beta1^3)) /
    sqrt((1 - beta2) / (1 - beta2^3)) = 0.639 of that; for a first appearance at step t the factor is that expression
    with t in place of 3 (0.98 at t = 100, 2.5 at t = 1000, towards (1 - beta1) / sqrt(1 - beta2) = 3.16), and the
    parameter's next steps differ from torch's likewise until its own moments have filled."""

    def __init__(self, model, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-7, max_norm=35.0, ema_decay=0.9990,
                 ema_updates=0, loss_scale=None):
        self.model = model
        self.params, seen = [], set()
        for p in model.parameters():
            if id(p) not in seen:
                seen.add(id(p))
                self.params.append(p)
        if not self.params:
            raise ValueError("ParamUpdate: the model has no parameters")
        for p in self.params:
            if not p.is_cuda:
                raise _capi.VampireHipError("ParamUpdate needs device parameters (no CPU fallback)")
            if p.dtype != torch.float32:
                raise TypeError(f"ParamUpdate takes fp32 parameters, got {p.dtype}")
            if not p.is_contiguous():
                raise ValueError("ParamUpdate takes contiguous parameters")
        self.device = self.params[0].device
        if any(p.device != self.device for p in self.params):
            raise ValueError("ParamUpdate: all parameters must live on one device")
        self.use_ema = ema_decay is not None and ema_decay > 0
        # the state_dict's entries: key -> index into self._tensors (float entries), or a copy (the others)
        self._tensors, self._slot_of_key, self._frozen = list(self.params), collections.OrderedDict(), {}
        index = {id(p): i for i, p in enumerate(self.params)}
        for key, v in model.state_dict(keep_vars=True).items():
            if not v.dtype.is_floating_point:
                self._frozen[key] = v.detach().clone()          # the reference's deep copy never updates them
                self._slot_of_key[key] = None
                continue
            if id(v) not in index:
                if v.dtype != torch.float32 or v.device != self.device or not v.is_contiguous():
                    raise TypeError(f"ParamUpdate: buffer {key} must be a contiguous fp32 tensor on {self.device}")
                index[id(v)] = len(self._tensors)
                self._tensors.append(v)
            self._slot_of_key[key] = index[id(v)]
        kinds = [KIND_PARAM] * len(self.params) + [KIND_EMA_ONLY] * (len(self._tensors) - len(self.params))
        self.plan = plan_update([t.numel() for t in self._tensors], kinds, UPDATE_CHUNK)
        pl = self.plan
        mode = _capi.VAMP_UPDATE_SCALE_NONE
        scale = 1.0
        if isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError(f'loss_scale must be None, a number or "dynamic", got {loss_scale!r}')
            mode, scale = _capi.VAMP_UPDATE_SCALE_DYNAMIC, INITIAL_SCALE
        elif loss_scale is not None:
            mode, scale = _capi.VAMP_UPDATE_SCALE_STATIC, float(loss_scale)
            if not (scale > 0 and np.isfinite(scale)):
                raise ValueError(f"loss_scale must be positive and finite, got {loss_scale}")
        self.desc = _capi.VampParamUpdateDesc(float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                                              float(max_norm) if max_norm is not None else 0.0,
                                              float(ema_decay) if self.use_ema else 0.0,
                                              pl.n_param_chunks, pl.n_buffer_chunks, mode, 0)
        vamp = _capi.checked()
        need = vamp.vamp_param_update_workspace_bytes(self.desc)
        if need == 0:
            raise refused(vamp, "ParamUpdate")
        dev = self.device
        with torch.cuda.device(dev):
            self.exp_avg = torch.zeros(pl.param_state, dtype=torch.float32, device=dev)
            self.exp_avg_sq = torch.zeros(pl.param_state, dtype=torch.float32, device=dev)
            self.ema = torch.zeros(pl.total_state if self.use_ema else 0, dtype=torch.float32, device=dev)
            if self.use_ema:
                with torch.no_grad():
                    for t, v in zip(self._tensors, self._ema_views()):
                        v.copy_(t.detach())
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
            host = _capi.VampUpdateScalars(lr=float(lr), step=0, updates=int(ema_updates), scale=scale)
            words = np.frombuffer(bytes(host), dtype=np.int32).copy()
            assert words.size == _SCALAR_WORDS
            self._scalars = torch.from_numpy(words).to(dev)
            n_chunks = pl.n_param_chunks + pl.n_buffer_chunks
            self._table = torch.zeros(n_chunks * CHUNK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self._f32, self._i64 = self._scalars.view(torch.float32), self._scalars.view(torch.int64)
        self._f64 = self._scalars.view(torch.float64)
        self._elem_bytes = pl.offset * 4
        self._base = np.array([t.data_ptr() for t in self._tensors], dtype=np.uint64)
        self._is_param_chunk = pl.kind == KIND_PARAM
        self._grad_ptrs = None            # what the device table holds; None: nothing uploaded yet
        self._uploads = []                # (pinned table, event): alive until the copy has passed

    # ------------------------------------------------------------------ state
    def _ema_views(self):
        pl = self.plan
        return [self.ema[o:o + t.numel()].view(t.shape) for t, o in zip(self._tensors, pl.tensor_state_offset.tolist())]

    @property
    def stats(self):
        """Device tensors (0-dim views of the scalar block, valid after every step without a synchronisation):
        total_norm (of the unscaled gradients), clip_coef, found_inf, step (t), updates (n), scale (the loss scale the
        NEXT backward is to use)."""
        f, i, w = self._f32, self._scalars, self._i64
        return {"total_norm": f[_W["total_norm"]], "clip_coef": f[_W["clip_coef"]], "found_inf": i[_W["found_inf"]],
                "step": w[_W["step"] // 2], "updates": w[_W["updates"] // 2], "scale": f[_W["scale"]]}

    def set_lr(self, lr):
        """The learning rate of the following steps (a fill of the device scalar: it does not block)."""
        self._f64[_W["lr"] // 2].fill_(float(lr))

    def scale_loss(self, loss):
        """loss times the device loss scale (1 without loss scaling): call backward() on the result."""
        return loss * self._f32[_W["scale"]]

    def zero_grad(self, set_to_none=True):
        if set_to_none:
            for p in self.params:
                p.grad = None
            return
        grads = [p.grad for p in self.params if p.grad is not None]
        for g in grads:
            g.detach_()
            g.requires_grad_(False)
        if grads:
            torch._foreach_zero_(grads)

    def ema_state_dict(self):
        """The averaged weights under the keys of model.state_dict(): float entries are views of the flat EMA (they
        follow later steps), the others the values copied at construction."""
        if not self.use_ema:
            raise RuntimeError("ParamUpdate was built without an EMA (ema_decay <= 0)")
        views = self._ema_views()
        return collections.OrderedDict((k, self._frozen[k] if s is None else views[s])
                                       for k, s in self._slot_of_key.items())

    def copy_ema_to(self, module):
        """Load the averaged weights into `module` (a model of the same architecture)."""
        return module.load_state_dict(self.ema_state_dict())

    def state_dict(self):
        return {"exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(), "ema": self.ema.clone(),
                "scalars": self._scalars.clone(), "numels": [t.numel() for t in self._tensors],
                "chunk": UPDATE_CHUNK}

    def load_state_dict(self, state):
        if list(state["numels"]) != [t.numel() for t in self._tensors]:
            raise ValueError("ParamUpdate.load_state_dict: the state belongs to a model with other tensor sizes")
        for name in ("exp_avg", "exp_avg_sq", "ema"):
            dst, src = getattr(self, name), state[name]
            if dst.shape != src.shape:
                raise ValueError(f"ParamUpdate.load_state_dict: {name} has {tuple(src.shape)}, expected {tuple(dst.shape)}")
            dst.copy_(src)
        self._scalars.copy_(state["scalars"])

    # ------------------------------------------------------------------ the step
    def _upload(self, ptrs):
        pl = self.plan
        for p, a in zip(self.params, ptrs):
            if a:
                g = p.grad
                if g.dtype != torch.float32:
                    raise TypeError(f"ParamUpdate takes fp32 gradients, got {g.dtype}")
                if g.device != self.device or g.shape != p.shape or not g.is_contiguous() or g.is_sparse:
                    raise ValueError("ParamUpdate: a gradient must be a dense contiguous tensor of its parameter's shape "
                                     "on the parameter's device")
        gbase = np.zeros(len(self._tensors), dtype=np.uint64)
        gbase[:len(ptrs)] = ptrs
        has = gbase[pl.tensor] != 0
        host = np.zeros(len(pl.tensor), dtype=CHUNK_DTYPE)
        host["param"] = self._base[pl.tensor] + self._elem_bytes.astype(np.uint64)
        host["grad"] = np.where(has, gbase[pl.tensor] + self._elem_bytes.astype(np.uint64), np.uint64(0))
        host["state_off"] = pl.state_offset
        host["len"] = pl.length
        host["kind"] = np.where(has & self._is_param_chunk, KIND_PARAM, KIND_EMA_ONLY)
        self._uploads = [(t, ev) for t, ev in self._uploads if not ev.query()]
        pinned = torch.empty(host.nbytes, dtype=torch.uint8).pin_memory()
        pinned.numpy()[:] = host.view(np.uint8).reshape(-1)
        self._table.copy_(pinned, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._uploads.append((pinned, ev))
        self._grad_ptrs = ptrs

    @torch.no_grad()
    def step(self):
        ptrs = [0 if p.grad is None else p.grad.data_ptr() for p in self.params]
        with torch.cuda.device(self.device):
            if ptrs != self._grad_ptrs:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(
                        "ParamUpdate.step(): a gradient's address differs from the chunk table's during a stream "
                        "capture; run one eager step() on these gradient tensors first and keep them with "
                        "zero_grad(set_to_none=False)")
                self._upload(ptrs)
            _capi.checked().vamp_param_update_step(self.desc, self._table, self.exp_avg, self.exp_avg_sq,
                                                   self.ema if self.use_ema else None, self._scalars, self._ws,
                                                   self._ws.numel(), _stream())
