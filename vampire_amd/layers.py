"""Layer operators on plain tensors (Python over the C ABI): the free functions a network calls without a `HotPath`
-- BEVDepth voxel pooling, the trilinear resize and 3x3x3 convolutions of the 3-D UNet, and the 2-D bilinear resize of
the rendered maps, with autograd support.
All work happens in hand-written HIP kernels reached through `_capi`; there is no CPU fallback."""
import math
from typing import NamedTuple

import torch

from . import _capi
from ._tensors import (DTYPE_CODES, FLOAT_DTYPES, HALF_DTYPES, _accept, _aligned, _chk, _dtype_code, _stream,
                       need_device, scratch)


# ===========================================================================
# BEVDepth-style voxel pooling (north_star; SURVEY 8 row a11 -- not in the reference tree, parity unpinned)
# ===========================================================================
def voxel_pooling(geom_xyz, input_features, voxel_num):
    """The published BEVDepth operator `voxel_pooling(geom_xyz, input_features, voxel_num)`:
    geom_xyz [B, N, D, H, W, 3] integer voxel indices (x, y, z), input_features [B, N, D, H, W, C]
    (fp32 | bf16), voxel_num (nx, ny, nz) -> [B, C, ny, nx] fp32, the sum of the features of the points
    falling into each BEV cell (points outside the grid are dropped).  HIP kernels, no CPU fallback."""
    return _VoxelPoolingFn.apply(geom_xyz, input_features, tuple(int(v) for v in voxel_num))


class _VoxelPoolingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, geom, feat, voxel_num):
        need_device("voxel_pooling", geom, feat)
        vamp = _capi.checked()
        B, C_ = feat.shape[0], feat.shape[-1]
        P = feat[0].numel() // C_
        ctx.in_dtype, ctx.fshape = feat.dtype, tuple(feat.shape)
        feat = _aligned(_accept(feat).reshape(B, P, C_))
        geom = _aligned(_chk(geom.reshape(B, P, 3).to(torch.int32), (B, P, 3), "geom_xyz"))
        d = _capi.VampPoolDesc(B, C_, P, voxel_num[0], voxel_num[1], voxel_num[2], _dtype_code(feat))
        out = torch.empty(B, voxel_num[1], voxel_num[0], C_, dtype=torch.float32, device=feat.device)
        ws = scratch("voxel_pooling", feat.device, vamp.vamp_voxel_pooling_workspace_bytes(d))
        with torch.cuda.device(feat.device):
            vamp.vamp_voxel_pooling_forward(d, geom, feat, out, ws, ws.numel(), _stream())
        ctx.desc = d
        ctx.save_for_backward(geom)
        return out.permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, g):
        (geom,) = ctx.saved_tensors
        d = ctx.desc
        g = _aligned(g.permute(0, 2, 3, 1).float())
        gfeat = torch.empty(d.B, d.P, d.C, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            _capi.checked().vamp_voxel_pooling_backward(d, geom, g, gfeat, _stream())
        return None, gfeat.reshape(ctx.fshape).to(ctx.in_dtype), None


# ===========================================================================
# trilinear resize of the 3-D UNet (first piece)
# ===========================================================================
def upsample_trilinear(x, size):
    """F.interpolate(x, size, mode='trilinear', align_corners=True) (bv2:66, 72) on the HIP
    kernels: x [B,C,z,y,x] fp32 device tensor -> [B,C,*size]; the backward is a gather (aten's
    float-atomic scatter takes 2.2 ms per call at the UNet's full-resolution level)."""
    return _UpsampleTrilinearFn.apply(x, tuple(int(v) for v in size))


class _UpsampleTrilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, size):
        if not x.is_cuda:
            raise _capi.VampireHipError("x must be a device tensor (no CPU fallback)")
        if x.dim() != 5 or len(size) != 3:
            raise ValueError("expected a [B,C,z,y,x] tensor and a 3-tuple size")
        vamp = _capi.checked()
        ctx.in_dtype = x.dtype
        if x.dtype not in FLOAT_DTYPES:
            x = x.float()
        x = _aligned(x)
        ctx.code = DTYPE_CODES[x.dtype]
        B, C_ = x.shape[:2]
        ctx.dtype = x.dtype
        out = torch.empty((B, C_) + size, dtype=x.dtype, device=x.device)
        if out.numel() and x.numel():
            vamp.vamp_upsample_trilinear_forward_ex(B * C_, *x.shape[2:], *size, ctx.code, x, out, _stream())
        ctx.vamp, ctx.dims = vamp, (B * C_,) + tuple(x.shape[2:]) + size
        ctx.in_shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        dt = ctx.dtype
        g = _aligned(g.to(dt))
        gin = torch.empty(ctx.in_shape, dtype=dt, device=g.device)
        if gin.numel() and g.numel():
            vamp = ctx.vamp
            nbytes = vamp.vamp_upsample_trilinear_workspace_bytes(*ctx.dims[1:4])
            ws = scratch("upsample_trilinear", g.device, nbytes, per_size=True)         # (one table per size)
            vamp.vamp_upsample_trilinear_backward_ex(*ctx.dims, ctx.code, g, gin, ws, ws.numel(), _stream())
        else:
            gin.zero_()
        return gin.to(ctx.in_dtype), None


# ===========================================================================
# 2-D bilinear resize of the rendered maps (bv2:616-626, 203-209)
# ===========================================================================
def resize_bilinear2d(x, size):
    """F.interpolate(x, size, mode='bilinear', align_corners=True) on the HIP kernels: x [..., H, W] fp32 device tensor
    -> [..., *size].  The backward is a gather in a fixed order (aten's scatters with float atomics), so gradients are
    bitwise repeatable.  Sizes `vamp_resize2d_supported` refuses raise; the caller decides what to do with them."""
    return resize_bilinear2d_pack([x], size)[0]


def resize_bilinear2d_pack(tensors, size):
    """The same for up to 4 tensors that share H and W (leading dimensions are free: the camera maps' 3, num_classes
    and 1 channels), in one launch forward and one backward.  Returns a list.  An output that receives no gradient is
    left out of the backward launch."""
    return list(_Resize2dFn.apply(tuple(int(v) for v in size), *tensors))


def resize_bilinear2d_supported(in_size, size) -> bool:
    return bool(_capi.checked().vamp_resize2d_supported(*(int(v) for v in in_size), *(int(v) for v in size)))


def _resize2d_desc(ih, iw, oh, ow, pairs) -> _capi.VampResize2dDesc:
    """pairs: (src, dst) tensors per segment; the planes are whatever leads the two resized axes."""
    d = _capi.VampResize2dDesc()
    d.ih, d.iw, d.oh, d.ow, d.nseg = ih, iw, oh, ow, len(pairs)
    for k, (src, dst) in enumerate(pairs):
        d.seg[k].src, d.seg[k].dst = src.data_ptr(), dst.data_ptr()
        d.seg[k].planes = src.numel() // (src.shape[-1] * src.shape[-2])
    return d


class _Resize2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, size, *tensors):
        if not 1 <= len(tensors) <= _capi.VAMP_RESIZE2D_MAX_SEGS:
            raise ValueError(f"expected 1 to {_capi.VAMP_RESIZE2D_MAX_SEGS} tensors, got {len(tensors)}")
        if len(size) != 2:
            raise ValueError("size must be (H, W)")
        for t in tensors:
            need_device("resize_bilinear2d", t)
            if t.dim() < 2 or t.dtype != torch.float32 or t.numel() == 0:
                raise ValueError("expected non-empty fp32 tensors [..., H, W]")
            if tuple(t.shape[-2:]) != tuple(tensors[0].shape[-2:]) or t.device != tensors[0].device:
                raise ValueError("the tensors of a pack share H, W and the device")
        ih, iw = tensors[0].shape[-2:]
        xs = [_aligned(t) for t in tensors]
        outs = [torch.empty(tuple(t.shape[:-2]) + size, dtype=torch.float32, device=t.device) for t in tensors]
        with torch.cuda.device(xs[0].device):
            _capi.checked().vamp_resize2d_forward(_resize2d_desc(ih, iw, *size, list(zip(xs, outs))), _stream())
        ctx.dims = (ih, iw) + size
        ctx.in_shapes = [tuple(t.shape) for t in tensors]
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        vamp = _capi.checked()
        pairs, gins = [], [None] * len(grads)
        for k, g in enumerate(grads):
            if g is None or not ctx.needs_input_grad[1 + k]:
                continue                    # no gradient came for this output: its segment is not launched
            gins[k] = torch.empty(ctx.in_shapes[k], dtype=torch.float32, device=g.device)
            pairs.append((_aligned(g.float()), gins[k]))
        if pairs:
            dev = pairs[0][0].device
            nbytes = vamp.vamp_resize2d_workspace_bytes(*ctx.dims)
            ws = scratch("resize2d", dev, nbytes) if nbytes else None
            with torch.cuda.device(dev):
                vamp.vamp_resize2d_backward(_resize2d_desc(*ctx.dims, pairs), ws, nbytes, _stream())
        return (None,) + tuple(gins)


# ===========================================================================
# 3x3x3 convolutions of the 3-D UNet
# ===========================================================================
def _conv_desc(x_shape, w_shape) -> _capi.VampConvDesc:
    d = _capi.VampConvDesc()
    d.B, d.cin, d.Z, d.Y, d.X = x_shape
    d.cout = w_shape[0]
    return d


class _ConvKind(NamedTuple):
    """A row per convolution: the public name, the entry points' stem (+ forward / backward_data / backward_weight),
    the workspace's size function and tag, the library's shape rule, the stride, `half` (16-bit operands: a dtype
    code goes to the entry points and the fp32 weight gradient is cast back to the weight's dtype), and whether a
    wrong dtype or rank is refused before a host tensor."""
    name: str
    stem: str
    workspace_bytes: str
    tag: str
    supported: str
    stride: int
    half: bool
    dtype_first: bool = False


_CONV_KINDS = {
    "fp32": _ConvKind("conv3d_3x3x3", "vamp_conv3d_", "vamp_conv3d_workspace_bytes", "conv", "vamp_conv3d_supported",
                      1, False),
    "half": _ConvKind("conv3d_bf16", "vamp_conv3d_half_", "vamp_conv3d_bf16_workspace_bytes", "conv16",
                      "vamp_conv3d_bf16_supported", 1, True),
    "half_s2": _ConvKind("conv3d_bf16_stride2", "vamp_conv3d_half_s2_", "vamp_conv3d_half_s2_workspace_bytes",
                         "conv16s2", "vamp_conv3d_half_s2_supported", 2, True, dtype_first=True),
}


def _conv3d_layer_ok(kind, x_shape, w_shape, on_device, stride, padding, has_bias) -> bool:
    """nn.Conv3d(cin, cout, 3, the kind's stride, 1, bias=False) on a device tensor whose volume the kind's kernels
    take (the library's answer, which needs no GPU).  Dtypes and autocast are the caller's."""
    k = _CONV_KINDS[kind]
    if not (on_device and not has_bias and tuple(stride) == (k.stride,) * 3 and tuple(padding) == (1, 1, 1)
            and tuple(w_shape[2:]) == (3, 3, 3) and len(x_shape) == 5 and w_shape[1] == x_shape[1]):
        return False
    return bool(getattr(_capi.checked(), k.supported)(_conv_desc(x_shape, w_shape)))


def conv3d_kind(x_shape, w_shape, x_dtype, w_dtype, on_device, stride, padding, has_bias, autocast=None, min_voxels=0,
                stride2=True):
    """Which convolution runs a layer, from plain values: "fp32", "half", "half_s2" or None (aten / MIOpen).
    `autocast` is the dtype of the enabled CUDA autocast or None.  Under a 16-bit one the operands are cast to it,
    whatever they are: the stride-1 kernels, else (`stride2`, the switch) the stride-2 ones; `min_voxels` does not
    apply.  Under no autocast at all: fp32 tensors of at least `min_voxels` voxels per channel, stride 1."""
    layer = (tuple(x_shape), tuple(w_shape), on_device, stride, padding, has_bias)
    if autocast in HALF_DTYPES:
        if _conv3d_layer_ok("half", *layer):
            return "half"
        return "half_s2" if stride2 and _conv3d_layer_ok("half_s2", *layer) else None
    if (autocast is None and x_dtype == w_dtype == torch.float32 and _conv3d_layer_ok("fp32", *layer)
            and math.prod(x_shape[2:]) >= min_voxels):
        return "fp32"
    return None


def cuda_autocast():
    """The dtype of the enabled CUDA autocast (the reference trains with Lightning's `precision=16`), else None."""
    return torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else None


def conv3d_supported(x, weight, stride, padding, bias):
    return conv3d_kind(x.shape, weight.shape, x.dtype, weight.dtype, x.is_cuda, stride, padding, bias is not None,
                       autocast=cuda_autocast()) == "fp32"


def _half_supported(kind, x, weight, stride, padding, bias):
    return x.dtype in HALF_DTYPES and _conv3d_layer_ok(kind, x.shape, weight.shape, x.is_cuda, stride, padding,
                                                       bias is not None)


def conv3d_bf16_supported(x, weight, stride, padding, bias):
    return _half_supported("half", x, weight, stride, padding, bias)


def conv3d_bf16_stride2_supported(x, weight, stride, padding, bias):
    return _half_supported("half_s2", x, weight, stride, padding, bias)


def conv3d_3x3x3(x, weight):
    """nn.Conv3d(cin, cout, 3, 1, 1, bias=False) (bv2:20, 40-60) on the fp32 matrix cores:
    x [B,cin,Z,Y,X], weight [cout,cin,3,3,3], cin / cout in {16, 32}; fp32 device tensors."""
    return _Conv3dFn.apply("fp32", x, weight)


def conv3d_bf16(x, weight):
    """The same layer in bf16 (what the reference's `precision=16` training hands it): x bf16 [B,cin,Z,Y,X],
    weight bf16 [cout,cin,3,3,3] -> bf16 [B,cout,Z,Y,X]; fp32 accumulation on the bf16 matrix cores."""
    return _Conv3dFn.apply("half", x, weight)


def conv3d_bf16_stride2(x, weight):
    """nn.Conv3d(cin, cout, 3, stride=2, padding=1, bias=False) (Hourglass3D.conv1 / conv3, bv2:34-46) in bf16 or
    fp16: x [B,cin,Z,Y,X], weight [cout,cin,3,3,3] of the same 16-bit dtype -> [B,cout,(Z-1)//2+1,(Y-1)//2+1,X//2];
    fp32 accumulation on the 16-bit matrix cores."""
    return _Conv3dFn.apply("half_s2", x, weight)


def _conv_operands(kind, x, w, others=None):
    """The operand side of both autograd functions.  Refusals, in order: a host tensor, then a wrong dtype.  The plain
    wrappers (`others` None) refuse a wrong rank with the dtype, and a `dtype_first` kind of theirs refuses both
    before a host tensor; the epilogue (`others`: its further tensors) has texts of its own and leaves the rank to
    `_epi_kind`.  Returns the kind's row, the aligned operands, the descriptor (it holds the input volume), the output
    volume and the dtype code the kind's entry points take."""
    k = _CONV_KINDS[kind]
    bad_dtype = x.dtype not in (HALF_DTYPES if k.half else (torch.float32,)) or w.dtype != x.dtype
    if others is not None:                         # the epilogue
        if not (x.is_cuda and w.is_cuda and all(t.is_cuda for t in others)):
            raise _capi.VampireHipError("conv3d epilogue: device tensors only (no CPU fallback)")
        if bad_dtype:
            raise TypeError(f"the {kind} kind takes {'bf16 or fp16' if k.half else 'fp32'} operands of one dtype")
    else:                                          # the plain wrappers
        on_host = not (x.is_cuda and w.is_cuda)
        if on_host and not k.dtype_first:
            raise _capi.VampireHipError("x / weight must be device tensors (no CPU fallback)")
        if bad_dtype or x.dim() != 5 or w.dim() != 5:
            raise TypeError(f"{k.name} takes {'bf16 (or fp16)' if k.half else 'fp32'} [B,cin,Z,Y,X] and "
                            f"[cout,cin,3,3,3] tensors{' of one dtype' if k.half else ''}")
        if on_host:
            raise _capi.VampireHipError("x / weight must be device tensors (no CPU fallback)")
    _capi.checked()
    x, w = _aligned(x), _aligned(w)
    d = _conv_desc(x.shape, w.shape)
    if w.shape[1] != d.cin:
        raise ValueError("weight / input channel mismatch")
    vol = tuple((n - 1) // k.stride + 1 for n in (d.Z, d.Y, d.X))
    return k, x, w, d, vol, ((DTYPE_CODES[x.dtype],) if k.half else ())


def _conv_backward(k, d, code, x, w, gz, need_x, need_w):
    """The convolution's own backward from the aligned gradient `gz` of its output: (gx, gw), None where not needed."""
    vamp = _capi.checked()
    gx = gw = None
    if need_x:
        gx = torch.empty_like(x)
        getattr(vamp, k.stem + "backward_data")(d, *code, gz, w, gx, _stream())
    if need_w:
        gw = torch.empty(w.shape, dtype=torch.float32, device=w.device)
        nbytes = getattr(vamp, k.workspace_bytes)(d)
        ws = scratch(k.tag, gz.device, nbytes, per_size=True)
        getattr(vamp, k.stem + "backward_weight")(d, *code, x, gz, gw, ws, ws.numel(), _stream())
        if k.half:
            gw = gw.to(w.dtype)                   # the gradient of the 16-bit copy autocast made of the fp32 parameter
    return gx, gw


class _Conv3dFn(torch.autograd.Function):
    """The three convolutions, told apart by their row of `_CONV_KINDS`."""

    @staticmethod
    def forward(ctx, kind, x, w):
        k, x, w, d, vol, ctx.code = _conv_operands(kind, x, w)
        out = torch.empty((d.B, d.cout) + vol, dtype=x.dtype, device=x.device)
        getattr(_capi.checked(), k.stem + "forward")(d, *ctx.code, x, w, out, _stream())
        ctx.desc, ctx.kind = d, k
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        gx, gw = _conv_backward(ctx.kind, ctx.desc, ctx.code, x, w, _aligned(g.to(x.dtype)), *ctx.needs_input_grad[1:])
        return None, gx, gw


# ===========================================================================
# the same convolutions with an epilogue: y = act(conv(x, w) + bias + residual)  (conv3d_epilogue.hpp)
# ===========================================================================
_ACT_CODES = {None: _capi.VAMP_ACT_NONE, "none": _capi.VAMP_ACT_NONE, "leaky_relu": _capi.VAMP_ACT_LEAKY_RELU,
              "sigmoid": _capi.VAMP_ACT_SIGMOID}


class HeadSegment(NamedTuple):
    """A run of consecutive output channels of `conv3d_heads`: its channel count, fp32 bias [channels] or None, the
    activation (None, "leaky_relu", "sigmoid"), the output dtype (None: the operands'; torch.float32 from 16-bit
    operands) and leaky_relu's slope.  The segments follow one another from channel 0."""
    channels: int
    bias: object = None
    act: object = None
    out_dtype: object = None
    negative_slope: float = 0.01


class _EpiSeg(NamedTuple):
    """A segment as `_Conv3dEpiFn` takes it (plain values; the tensors travel as arguments of `apply`)."""
    c0: int
    nch: int
    act: int
    slope: float
    out_f32: bool
    has_bias: bool
    has_residual: bool


def _epi_kind(x, weight, stride):
    """The kind `conv3d_kind` names for the layer (a bias is no refusal here), the 16-bit dtype its operands are cast
    to (None: fp32).  Outside an autocast, 16-bit operands choose their own dtype.  No kind: an error."""
    if not (x.is_cuda and weight.is_cuda):
        raise _capi.VampireHipError("x / weight must be device tensors (no CPU fallback)")
    if x.dim() != 5 or weight.dim() != 5:
        raise TypeError("expected [B,cin,Z,Y,X] and [cout,cin,3,3,3] tensors")
    ac = cuda_autocast()
    if ac is None:
        if x.dtype != weight.dtype or x.dtype not in FLOAT_DTYPES:
            raise TypeError(f"x / weight must share fp32, bf16 or fp16, got {x.dtype} and {weight.dtype}")
        if x.dtype in HALF_DTYPES:
            ac = x.dtype
    kind = conv3d_kind(x.shape, weight.shape, x.dtype, weight.dtype, True, (stride,) * 3, (1, 1, 1), False, autocast=ac)
    if kind is None:
        raise _capi.VampireHipError(f"no HIP convolution takes x {tuple(x.shape)} {x.dtype}, weight "
                                    f"{tuple(weight.shape)}, stride {stride} (no fallback)")
    return kind, (ac if kind != "fp32" else None)


def _epi_desc(segs, bias=(), residual=(), out=(), grad_out=(), grad_bias=()) -> _capi.VampConvEpilogue:
    e = _capi.VampConvEpilogue()
    e.nseg = len(segs)
    ptr = lambda seq, k: seq[k].data_ptr() if k < len(seq) and seq[k] is not None else None
    for k, s in enumerate(segs):
        g = e.seg[k]
        g.c0, g.nch, g.act, g.out_f32, g.slope = s.c0, s.nch, s.act, int(s.out_f32), s.slope
        g.bias, g.residual, g.out = ptr(bias, k), ptr(residual, k), ptr(out, k)
        g.grad_out, g.grad_bias = ptr(grad_out, k), ptr(grad_bias, k)
    return e


def conv3d_fused(x, weight, bias=None, residual=None, act=None, negative_slope=0.01, stride=1):
    """act(conv3d(x, weight, stride, padding=1) + bias + residual) in ONE kernel and one autograd node: the 3x3x3
    convolution `conv3d_kind` names for the operands (under a 16-bit autocast they are cast to it), with the bias
    [cout], the residual (the output's shape; cast to its dtype) and the activation (None, "leaky_relu", "sigmoid")
    applied to the fp32 accumulator before the one rounding of the store.  No fallback: operands no kind takes raise."""
    if act not in _ACT_CODES:
        raise ValueError(f"act must be one of {sorted(k for k in _ACT_CODES if k)} or None, got {act!r}")
    kind, dt16 = _epi_kind(x, weight, stride)
    if dt16 is not None:
        x, weight = x.to(dt16), weight.to(dt16)
    if residual is not None:
        residual = residual.to(x.dtype)
    seg = _EpiSeg(0, weight.shape[0], _ACT_CODES[act], float(negative_slope), False, bias is not None,
                  residual is not None)
    extra = [t for t in (bias, residual) if t is not None]
    return _Conv3dEpiFn.apply(kind, (seg,), x, weight, *extra)[0]


def conv3d_heads(x, weight, segments, stride=1):
    """One convolution (stride 1, or 2 for 16-bit operands) whose output channels leave as several tensors: `segments` is 1 to 4 `HeadSegment`s
    (or tuples in its field order) that follow one another from channel 0; returns the tuple of their outputs
    [B, channels, Zo, Yo, Xo], each with its own bias, activation and dtype.  Channels of `weight` behind the last
    segment (the padding the fp32 kind's 16 / 32 channel counts need) are computed and not stored."""
    segments = [s if isinstance(s, HeadSegment) else HeadSegment(*s) for s in segments]
    if not 1 <= len(segments) <= _capi.VAMP_CONV_EPI_MAX_SEGS:
        raise ValueError(f"expected 1 to {_capi.VAMP_CONV_EPI_MAX_SEGS} segments, got {len(segments)}")
    kind, dt16 = _epi_kind(x, weight, stride)
    if dt16 is not None:
        x, weight = x.to(dt16), weight.to(dt16)
    segs, extra, c0 = [], [], 0
    for s in segments:
        if s.act not in _ACT_CODES:
            raise ValueError(f"unknown activation {s.act!r}")
        if s.out_dtype not in (None, x.dtype, torch.float32):
            raise TypeError(f"a segment's dtype is the operands' ({x.dtype}) or fp32, got {s.out_dtype}")
        segs.append(_EpiSeg(c0, int(s.channels), _ACT_CODES[s.act], float(s.negative_slope),
                            s.out_dtype == torch.float32 and x.dtype != torch.float32, s.bias is not None, False))
        if s.bias is not None:
            extra.append(s.bias)
        c0 += int(s.channels)
    if c0 > weight.shape[0]:
        raise ValueError(f"the segments hold {c0} channels, the weight {weight.shape[0]}")
    return _Conv3dEpiFn.apply(kind, tuple(segs), x, weight, *extra)


class _Conv3dEpiFn(torch.autograd.Function):
    """The three convolutions through their epilogue entry points.  `tensors`: per segment its bias, then its
    residual, where it has them.  Saved: x, w, and the outputs of the segments that have an activation."""

    @staticmethod
    def forward(ctx, kind, segs, x, w, *tensors):
        k, x, w, d, vol, code = _conv_operands(kind, x, w, tensors)
        it = iter(tensors)
        biases, residuals, outs, where = [], [], [], []
        for n, s in enumerate(segs):
            odt = torch.float32 if s.out_f32 else x.dtype
            b = r = None
            if s.has_bias:
                where.append((n, "bias"))
                b = next(it)
                if tuple(b.shape) != (s.nch,):
                    raise ValueError(f"bias: expected shape ({s.nch},), got {tuple(b.shape)}")
                b = _aligned(b.detach().float())
            if s.has_residual:
                where.append((n, "residual"))
                r = next(it)
                if tuple(r.shape) != (d.B, s.nch) + vol or r.dtype != odt:
                    raise ValueError(f"residual: expected {(d.B, s.nch) + vol} {odt}, got {tuple(r.shape)} {r.dtype}")
                r = _aligned(r.detach())
            biases.append(b)
            residuals.append(r)
            outs.append(torch.empty((d.B, s.nch) + vol, dtype=odt, device=x.device))
        epi = _epi_desc(segs, bias=biases, residual=residuals, out=outs)
        with torch.cuda.device(x.device):
            getattr(_capi.checked(), k.stem + "epilogue_forward")(d, *code, epi, x, w, _stream())
        ctx.desc, ctx.kind, ctx.segs, ctx.code, ctx.where = d, k, segs, code, where
        ctx.vol, ctx.tensor_dtypes = vol, [t.dtype for t in tensors]
        ctx.save_for_backward(x, w, *[o for o, s in zip(outs, segs) if s.act != _capi.VAMP_ACT_NONE])
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        x, w, *ys = ctx.saved_tensors
        d, k, segs = ctx.desc, ctx.kind, ctx.segs
        need = ctx.needs_input_grad
        none = (None,) * (4 + len(ctx.where))
        if all(g is None for g in grads) or not any(need):
            return none
        vamp = _capi.checked()
        dev = x.device
        want_bias = {n for j, (n, what) in enumerate(ctx.where) if what == "bias" and need[4 + j]}
        s0 = segs[0]
        plain = (len(segs) == 1 and s0.act == _capi.VAMP_ACT_NONE and not want_bias and not s0.out_f32
                 and s0.nch == d.cout)
        gbias = {}
        with torch.cuda.device(dev):
            if plain:                              # nothing between the gradient and the convolution's own backward
                gz = _aligned(grads[0].to(x.dtype))
            else:
                ys, gouts, youts = iter(ys), [], []
                for s, g in zip(segs, grads):
                    odt = torch.float32 if s.out_f32 else x.dtype
                    if g is None:
                        g = torch.zeros((d.B, s.nch) + ctx.vol, dtype=odt, device=dev)
                    gouts.append(_aligned(g.to(odt)))
                    youts.append(next(ys) if s.act != _capi.VAMP_ACT_NONE else None)
                gz = torch.empty((d.B, d.cout) + ctx.vol, dtype=x.dtype, device=dev)
                gbias = {n: torch.empty(segs[n].nch, dtype=torch.float32, device=dev) for n in want_bias}
                epi = _epi_desc(segs, out=youts, grad_out=gouts,
                                grad_bias=[gbias.get(n) for n in range(len(segs))])
                ws, nbytes = None, 0
                if want_bias:
                    nbytes = vamp.vamp_conv3d_epilogue_workspace_bytes(d, k.stride)
                    ws = scratch("convepi", dev, nbytes, per_size=True)
                vamp.vamp_conv3d_epilogue_backward(d, k.stride, DTYPE_CODES[x.dtype], epi, gz, ws, nbytes, _stream())
            gx, gw = _conv_backward(k, d, ctx.code, x, w, gz, need[2], need[3])
        extra = []
        for j, (n, what) in enumerate(ctx.where):
            s = segs[n]
            if not need[4 + j]:
                extra.append(None)
            elif what == "bias":
                extra.append(gbias[n].to(ctx.tensor_dtypes[j]))
            else:                                  # the residual's gradient is g_z itself (its segment's channels)
                g = gz if s.nch == d.cout else gz[:, s.c0:s.c0 + s.nch]
                extra.append(g.to(ctx.tensor_dtypes[j]))
        return (None, None, gx, gw) + tuple(extra)
