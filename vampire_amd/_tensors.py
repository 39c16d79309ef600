"""Tensor-side helpers every operator module shares (ops, layers, evaluation): what a kernel accepts, how a tensor is
checked before its address goes to the library, dtype and density codes, the current stream, scratch workspaces."""
import ctypes as C
import math

import torch

from . import _capi

# torch dtype -> VAMP_* code, for every dtype some entry point reads; each operator names the ones IT accepts
DTYPE_CODES = {torch.float32: _capi.VAMP_F32, torch.bfloat16: _capi.VAMP_BF16, torch.float16: _capi.VAMP_F16,
               torch.int64: _capi.VAMP_I64, torch.int32: _capi.VAMP_I32, torch.uint8: _capi.VAMP_U8}
HOT_PATH_DTYPES = (torch.float32, torch.bfloat16)
HALF_DTYPES = (torch.bfloat16, torch.float16)
FLOAT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _stream(stream=None):
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype not in HOT_PATH_DTYPES:
        raise TypeError(f"unsupported dtype {t.dtype}: the hot path takes fp32 or bf16 inputs")
    return DTYPE_CODES[t.dtype]


def _density_code(cfg) -> int:
    return _capi.VAMP_DENSITY_SDF_LAPLACE if cfg.density_mode == "sdf" else _capi.VAMP_DENSITY_SIGMOID


def _accept(t):
    """The kernels read fp32 or bf16; anything else (fp16 under the reference's precision=16
    autocast, base_cli.py:77, fp64) is promoted to fp32, as aten's autocast does for these ops."""
    if t is None or t.dtype in HOT_PATH_DTYPES:
        return t
    return t.float()


def _accept_float(t, name):
    """`_accept` for an operand that has to hold real numbers: an integer or bool tensor is a caller's mistake (labels,
    indices or a mask in a volume's place), not something to promote."""
    if t is not None and not t.is_floating_point():
        raise TypeError(f"{name}: expected a floating-point tensor, got {t.dtype}")
    return _accept(t)


def _is_channel_last(feat: torch.Tensor) -> bool:
    """feat [B, N, C, fH, fW] whose memory is [B, N, fH, fW, C] (a torch.channels_last producer's output, reshaped):
    what the lift wants -- it samples a pixel's C features as one run -- and takes zero-copy."""
    return (feat.dim() == 5 and feat.dtype == torch.float32 and feat.shape[2] > 1
            and feat.permute(0, 1, 3, 4, 2).is_contiguous() and feat.data_ptr() % 16 == 0)


def _needs_aligned_copy(t: torch.Tensor) -> bool:
    """True when `t` does not start on a 16-byte boundary (a view that begins at an odd element of a larger buffer):
    the layer kernels read their operands with 4-, 8- and 16-byte loads and assume the allocator's alignment."""
    return t.data_ptr() % 16 != 0


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """`t` contiguous and starting on a 16-byte boundary: itself when it already is, else a fresh copy (the guard the
    lift's zero-copy path has in `_is_channel_last`), so that no kernel ever sees a misaligned pointer."""
    t = t.contiguous()
    return t.clone() if _needs_aligned_copy(t) else t


def _logit_layout(x):
    """(layout, B, S, x) for logits [..., K]: rows when contiguous, planes when the memory is channel-first
    ([B, K, ...] behind a permute(0, 2, .., 1) view, the backbone's occ_logits; leading dimensions in front of the
    channel axis, as in the camera branch's [B, N, K, h, w], count into B), else a contiguous copy."""
    if x.is_contiguous():
        return _capi.VAMP_SEG_ROWS, 1, x.numel() // max(x.shape[-1], 1), x
    if x.dim() == 2 and x.t().is_contiguous():
        return _capi.VAMP_SEG_PLANES, 1, x.shape[0], x
    for k in range(1, x.dim() - 1):
        if x.movedim(-1, k).is_contiguous():
            return _capi.VAMP_SEG_PLANES, math.prod(x.shape[:k]), math.prod(x.shape[k:-1]), x
    x = x.contiguous()
    return _capi.VAMP_SEG_ROWS, 1, x.numel() // max(x.shape[-1], 1), x


def _chk(t: torch.Tensor, shape, name):
    if not t.is_cuda:
        raise _capi.VampireHipError(f"{name} must be a device tensor (no CPU fallback)")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t.contiguous()


def _mats(t: torch.Tensor, B, N, name):
    """Prepared camera matrices [B, N, 3, 4, 4] as the kernels read them: fp32, contiguous, and on a 16-byte boundary
    (the lift's camera cull loads whole matrix rows and the library refuses anything else).  48 floats per camera: the
    copy of a view that starts at an odd element costs nothing."""
    return _aligned(_chk(t.float(), (B, N, 3, 4, 4), name))


def _scalar(t: torch.Tensor, name):
    """A one-element device parameter (the learnable beta) as the kernels read it: fp32 [1], whatever shape, dtype or
    strides (an expanded tensor) the caller's has."""
    if not t.is_cuda:
        raise _capi.VampireHipError(f"{name} must be a device tensor (no CPU fallback)")
    if t.numel() != 1:
        raise ValueError(f"{name}: expected one element, got shape {tuple(t.shape)}")
    return t.reshape(1).float().contiguous()


def need_device(name, *tensors):
    """Raises unless every tensor is on a device; None is skipped, lists and tuples are walked."""
    for t in tensors:
        if isinstance(t, (list, tuple)):
            need_device(name, *t)
        elif t is not None and not t.is_cuda:
            raise _capi.VampireHipError(f"{name} needs device tensors (no CPU fallback)")


def as_mask(mask):
    """A mask as the kernels read it: bool (anything else is taken as `!= 0`), contiguous; None passes through."""
    return None if mask is None else (mask if mask.dtype == torch.bool else mask != 0).contiguous()


def as_labels(labels, dtypes):
    """Integer labels as the kernels read them: one of `dtypes` (anything else is cast to int64), contiguous."""
    return (labels if labels.dtype in dtypes else labels.long()).contiguous()


def check_out(x, shape, dtype, dev, name, *, align=0, terse=False):
    """`x`, a caller's output buffer, when it is a contiguous `shape` `dtype` tensor on `dev` (on an `align`-byte
    boundary), else ValueError.  `name` opens the text; the buffer is described as "name: (shape, dtype, device)", or,
    `terse`, as "name shape dtype" -- the sites' own wordings."""
    shape = tuple(shape)
    if x is None or tuple(x.shape) != shape or x.dtype != dtype or not x.is_contiguous() or x.device != dev \
            or (align and x.data_ptr() % align):
        if terse:
            got = f" {tuple(x.shape)} {x.dtype}"
        else:
            got = f": {None if x is None else (tuple(x.shape), x.dtype, x.device)}"
        how = f"contiguous, {align}-byte aligned" if align else "contiguous"
        raise ValueError(f"{name}{got} is not a {how} {shape} {dtype} on {dev}")
    return x


def refused(vamp, name, exc=ValueError):
    """The exception for a descriptor the library refused: `name` and the library's own sentence."""
    return exc(f"{name}: {vamp.vamp_last_error().decode('utf-8', 'replace')}")


def workspace_bytes(size_fn, desc, refuse):
    """size_fn(desc); where that is 0 -- a descriptor the library refuses -- `refuse()` first, the entry point's own
    call without operands, which raises with the entry point's name and the library's reason."""
    nbytes = size_fn(desc)
    if nbytes == 0:
        refuse()
    return nbytes


def list_dtype(tensors, name, dtype=None, what=None):
    """A per-sample list's dtype check: all `dtype` (spelt `what` in the text), or, without one, all alike."""
    got = {t.dtype for t in tensors}
    if dtype is None and len(got) != 1:
        raise TypeError(f"{name} must share one dtype, got {sorted(str(g) for g in got)}")
    if dtype is not None and got - {dtype}:
        raise TypeError(f"{name} must be {what}, got {sorted(str(g) for g in got)}")


def pad_lists(lists, fills=None, counts=False):
    """Per-sample lists of tensors [n_b, ...] (the lists agreeing on every n_b; a None list stays None) -> one padded
    [B, M, ...] tensor per list, `fills[i]` (0) behind each sample's rows, and with `counts` the int32 counts [B] on
    the samples' device.  The counts come from the shapes, one scalar fill per sample: nothing is read back from the
    device and nothing is copied to it."""
    pad = torch.nn.utils.rnn.pad_sequence
    out = tuple(None if l is None else pad(list(l), batch_first=True, padding_value=f)
                for l, f in zip(lists, fills or [0] * len(lists)))
    if counts:
        dev = lists[0][0].device
        out += (torch.stack([torch.full((), p.shape[0], dtype=torch.int32, device=dev) for p in lists[0]]),)
    return out


def _pad_samples(*lists):
    """pad_lists with zero fill and the counts: (one padded tensor per list ..., counts)."""
    return pad_lists(lists, counts=True)


_scratch = {}


def scratch(kind, device, nbytes, *, per_size=False):
    """The uninitialised uint8 workspace of the operator `kind` on `device`'s current stream, max(nbytes, 256) bytes
    when it is made.  Regrown when a call needs more (the old buffer goes back to the allocator), or, `per_size`, one
    buffer per size that is never regrown: DESIGN 8.26 says what either means under graph capture."""
    key = (kind, device, torch.cuda.current_stream(device).cuda_stream) + ((nbytes,) if per_size else ())
    ws = _scratch.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _scratch[key] = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
    return ws
