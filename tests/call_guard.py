"""A call guard for the hot path's C entry points: a proxy around the checked library (installed as `hp.vamp`) that
inspects every torch.Tensor argument BEFORE forwarding the call and raises ContractViolation without calling the
library when a tensor is not what the entry point will read -- wrong device, not contiguous, too few or too many
elements for the descriptor, an element size that disagrees with the dtype code of the call, a misaligned pointer where
the library states a requirement.  The ctypes binding converts and does not validate (`_capi.TensorPtr`), and a kernel
handed such a tensor returns different numbers, not an error: the guard is how the operator-contract tests see it.

TABLE maps (function, parameter name as spelled in include/vampire_hip.h) to what the header's comments say the
parameter holds; test_call_guard.py holds it against the header's prototypes."""
import math
import types

import torch

from vampire_amd import _capi, _header


class ContractViolation(Exception):
    """A tensor argument of a library call is not what the entry point reads; raised instead of making the call."""

    def __init__(self, function, parameter, reason):
        super().__init__(f"{function}({parameter}): {reason}")
        self.function, self.parameter, self.reason = function, parameter, reason


def header_prototypes():
    """{function: [(C type, parameter name)]} of every prototype in the header, as the package's reader gives them."""
    return {name: params for name, (_, params) in _header.read().prototypes.items()}


# C pointer type -> bytes per element, for the parameters whose type says it (void* parameters name their source below)
ELEMENT_BYTES = {"float": 4, "uint64_t": 8, "int16_t": 2, "uint8_t": 1, "uint32_t": 4, "int32_t": 4}
DTYPE_BYTES = {_capi.VAMP_F32: 4, _capi.VAMP_BF16: 2, _capi.VAMP_F16: 2}

# Pointer parameters of the covered functions that never carry a tensor:
EXCLUDED = {
    "d", "lift_desc",        # the descriptors: ctypes structures, passed by reference
    "stream", "wait_event",  # a hipStream_t / hipEvent_t handle
    "ozs_host",              # a HOST copy of the det-grid heights (a ctypes float array)
    "patch", "grid",         # int32_t[2] host arrays the cull-word query fills
}


def _desc(x):
    return getattr(x, "_obj", x)       # (a structure, or what ctypes.byref made of one)


def _ceil16(c):
    return (c + 15) // 16


# ---- what each parameter holds: a -> shape, `a` the call's arguments by header name with d = the descriptor -----------
def _lift(f):
    return lambda a: f(_desc(a.d))


_L_PIX = _lift(lambda d: (d.B, d.N, d.D, d.fH, d.fW))
_L_FEAT = _lift(lambda d: (d.B, d.N, d.C, d.fH, d.fW))
_L_OUT = _lift(lambda d: (d.B, d.C, d.Z, d.Y, d.X))
_L_VOX = _lift(lambda d: (d.B, d.N, d.Z, d.Y, d.X))
_L_DENSE = _lift(lambda d: (d.B, d.N, d.C, d.D, d.fH, d.fW))
_MATS = _lift(lambda d: (d.B, d.N, 3, 4, 4))

# spec: (shape function, where the element size of a void* parameter comes from | None, required alignment in bytes)
DESC, F32 = "d.in_dtype", None
LIFT = {
    "mats": (_MATS, F32, 16),                     # "mats must be 16-byte aligned (the cull reads whole matrix rows)"
    "xs": (_lift(lambda d: (d.X,)), F32, 0), "ys": (_lift(lambda d: (d.Y,)), F32, 0), "zs": (_lift(lambda d: (d.Z,)), F32, 0),
    "depth": (_L_PIX, DESC, 0),                   # depth [B, N, D, fH, fW]
    "feat": (_L_FEAT, DESC, 0),                   # feat [B, N, C, fH, fW]; [B, N, fH, fW, C] under *_FEAT_CHANNEL_LAST
    "logits": (_L_PIX, "logits_dtype", 0),
    "depth_out": (_L_PIX, F32, 0),
    "out": (_L_OUT, F32, 0), "grad_out": (_L_OUT, F32, 0),
    "hits": (_lift(lambda d: (d.B, d.Z, d.Y, d.X, _ceil16(d.C))), F32, 0),       # u64
    "grad_depth": (_L_PIX, F32, 0), "grad_feat": (_L_FEAT, F32, 0),
    "frustum_feats": (_L_DENSE, F32, 0), "grad_frustum_feats": (_L_DENSE, F32, 0),
    "valid": (_L_VOX, F32, 0), "ix0": (_L_VOX, F32, 0), "iy0": (_L_VOX, F32, 0), "iz0": (_L_VOX, F32, 0),
    "words": (lambda a: (_desc(a.d).B, _desc(a.d).Z, a.grid[1], a.grid[0]), F32, 0),
}
# the lift entry points read feat / write grad_feat pixel-major under these flags (16-byte aligned)
CHANNEL_LAST = {"vamp_lift_forward_ex": (_capi.VAMP_LIFTFWD_FEAT_CHANNEL_LAST, ("feat",)),
                "vamp_lift_forward_logits_ex": (_capi.VAMP_LIFTFWD_FEAT_CHANNEL_LAST, ("feat",)),
                "vamp_lift_backward_ex": (_capi.VAMP_LIFTBWD_FEAT_CHANNEL_LAST, ("feat", "grad_feat"))}

_R_VOL = lambda ch: _lift(lambda d: (d.B, ch(d), d.Z, d.Y, d.X))
_R_MAP = lambda ch: _lift(lambda d: (d.B, d.N, ch(d), d.fH, d.fW))
_R_BEV = lambda ch: _lift(lambda d: (d.B, ch(d), d.oY, d.oX))
_R_DET = lambda ch: _lift(lambda d: (d.B, ch(d), d.oZ, d.oY, d.oX))
_R_SMP = _lift(lambda d: (d.B, d.N, d.D - 1, d.fH, d.fW))
_one, _three = (lambda d: 1), (lambda d: 3)
_K, _C, _CO = (lambda d: d.K), (lambda d: d.C), (lambda d: d.C + (d.K if d.cat_seg else 0))
_BETA = (lambda a: (1,), F32, 0)
RENDER = {
    "geom": (_lift(lambda d: (d.B, d.N, d.D, d.fH, d.fW, 3)), F32, 0),
    "mats": (_MATS, F32, 0),
    "us": (_lift(lambda d: (d.fW,)), F32, 0), "vs": (_lift(lambda d: (d.fH,)), F32, 0), "ds": (_lift(lambda d: (d.D,)), F32, 0),
    "mids": (_lift(lambda d: (d.D - 1,)), F32, 0),
    "oxs": (_lift(lambda d: (d.oX,)), F32, 0), "oys": (_lift(lambda d: (d.oY,)), F32, 0),
    "ozs": (_lift(lambda d: (d.oZ,)), F32, 0), "bev_mids": (_lift(lambda d: (d.oZ,)), F32, 0),
    "beta": _BETA, "grad_beta": _BETA, "grad_beta_zero": _BETA,
    "density_feature": (_R_VOL(_one), DESC, 0), "semantic": (_R_VOL(_K), DESC, 0), "rgb": (_R_VOL(_three), DESC, 0),
    "base": (_R_VOL(_C), DESC, 0),
    "rgb_out": (_R_MAP(_three), F32, 0), "seg_out": (_R_MAP(_K), F32, 0), "depth_out": (_R_MAP(_one), F32, 0),
    "g_rgb": (_R_MAP(_three), F32, 0), "g_seg": (_R_MAP(_K), F32, 0), "g_depth": (_R_MAP(_one), F32, 0),
    "bev_rgb": (_R_BEV(_three), F32, 0), "bev_seg": (_R_BEV(_K), F32, 0), "bev_height": (_R_BEV(_one), F32, 0),
    "g_bev_rgb": (_R_BEV(_three), F32, 0), "g_bev_seg": (_R_BEV(_K), F32, 0), "g_bev_height": (_R_BEV(_one), F32, 0),
    "voxel_density": (_R_DET(_one), F32, 0), "voxel_output": (_R_DET(_CO), F32, 0),
    "g_voxel_density": (_R_DET(_one), F32, 0), "g_voxel_output": (_R_DET(_CO), F32, 0),
    "grad_density_feature": (_R_VOL(_one), F32, 0), "grad_semantic": (_R_VOL(_K), F32, 0),
    "grad_rgb": (_R_VOL(_three), F32, 0), "grad_base": (_R_VOL(_C), F32, 0),
    "inside": (_R_SMP, F32, 0), "ix0": (_R_SMP, F32, 0), "iy0": (_R_SMP, F32, 0), "iz0": (_R_SMP, F32, 0),
    "fxyz": (lambda a: _R_SMP(a) + (3,), F32, 0),
}
_S_VOL = _lift(lambda d: (d.B, d.C, d.Z, d.Y, d.X))
_S_OUT = lambda a: (_desc(a.d).B, _desc(a.d).C, a.points_per_sample)
SAMPLE = {
    "volume": (_S_VOL, DESC, 0), "beta": _BETA, "grad_beta": _BETA,
    "points": (lambda a: (_desc(a.d).B, a.points_per_sample, 3), F32, 0),
    "out": (_S_OUT, F32, 0), "grad_out": (_S_OUT, F32, 0), "grad_volume": (_S_VOL, F32, 0),
}
_SM = lambda a: (a.images, a.D, a.HW)
SOFTMAX = {"logits": (_SM, "in_dtype", 0), "depth": (_SM, F32, 0), "grad_depth": (_SM, F32, 0), "grad_logits": (_SM, F32, 0)}
_G_VO, _G_VD = (lambda a: (a.B, a.C, a.cells)), (lambda a: (a.B, 1, a.cells))
GATE = {"voxel_output": (_G_VO, F32, 0), "voxel_density": (_G_VD, F32, 0), "out": (_G_VO, F32, 0),
        "grad_out": (_G_VO, F32, 0), "grad_voxel_output": (_G_VO, F32, 0), "grad_voxel_density": (_G_VD, F32, 0)}
_GC_VO, _GC_VD = (lambda a: (a.B, a.C, a.oZ, a.cells)), (lambda a: (a.B, 1, a.oZ, a.cells))
_GC_W, _GC_B, _GC_OUT = (lambda a: (a.Cout, a.C * a.oZ)), (lambda a: (a.Cout,)), (lambda a: (a.B, a.Cout, a.cells))
GATE_CONV = {"voxel_output": (_GC_VO, F32, 0), "voxel_density": (_GC_VD, F32, 0), "weight": (_GC_W, F32, 0),
             "bias": (_GC_B, F32, 0), "out": (_GC_OUT, F32, 0), "grad_out": (_GC_OUT, F32, 0),
             "grad_voxel_output": (_GC_VO, F32, 0), "grad_voxel_density": (_GC_VD, F32, 0),
             "grad_weight": (_GC_W, F32, 0), "grad_bias": (_GC_B, F32, 0)}


# ---- workspaces: at least the bytes the matching *_workspace_bytes call returns ------------------------------------------
def _render_ws(q, a):
    n = q.vamp_render_workspace_bytes(a.d)
    save = {"vamp_render_camera_forward_ex": _capi.VAMP_CAMFWD_SAVE_SAMPLES,
            "vamp_render_forward_merged": _capi.VAMP_RENDERFWD_SAVE_SAMPLES}.get(a.function, 0)
    if save and (a.flags & save) and getattr(a, "geom", None) is None:
        n += q.vamp_render_samples_bytes(a.d)
    return n


WORKSPACE = {        # parameter -> (its size parameter, the bytes it needs)
    "lift": {"workspace": ("workspace_bytes", lambda q, a: q.vamp_lift_workspace_bytes(a.d))},
    "render": {"workspace": ("workspace_bytes", _render_ws),
               "lift_workspace": ("lift_workspace_bytes", lambda q, a: q.vamp_lift_workspace_bytes(a.lift_desc))},
    "bev": {"workspace": ("workspace_bytes", lambda q, a: q.vamp_render_bev_workspace_bytes(a.d))},
    "merged": {"workspace": ("workspace_bytes", _render_ws),
               "bev_workspace": ("bev_workspace_bytes", lambda q, a: q.vamp_render_bev_workspace_bytes(a.d))},
    "sample": {"workspace": ("workspace_bytes",
                             lambda q, a: q.vamp_sample_points_workspace_bytes(a.d, a.points_per_sample))},
    "gate_conv": {"workspace": ("workspace_bytes",
                                lambda q, a: q.vamp_gate_conv1x1_workspace_bytes(a.C, a.oZ, a.Cout))},
}

# function -> (the parameter specs of its family, its workspaces)
FUNCTIONS = {
    "vamp_lift_forward": (LIFT, "lift"), "vamp_lift_forward_ex": (LIFT, "lift"),
    "vamp_lift_forward_logits": (LIFT, "lift"), "vamp_lift_forward_logits_ex": (LIFT, "lift"),
    "vamp_lift_backward": (LIFT, "lift"), "vamp_lift_backward_ex": (LIFT, "lift"),
    "vamp_lift_finish_cells": (LIFT, "lift"),
    "vamp_lift_forward_dense": (LIFT, None), "vamp_lift_backward_dense": (LIFT, None),
    "vamp_lift_indices": (LIFT, None), "vamp_lift_cull_words": (LIFT, None),
    "vamp_render_camera_forward_ex": (RENDER, "render"), "vamp_render_camera_terminate": (RENDER, "render"),
    "vamp_render_camera_prepare_ex": (RENDER, "render"), "vamp_render_camera_prepare_with_lift": (RENDER, "render"),
    "vamp_render_camera_backward_acc": (RENDER, "render"),
    "vamp_render_forward_merged": (RENDER, "merged"),
    "vamp_render_bev_forward_ex": (RENDER, "bev"), "vamp_render_bev_backward_ex": (RENDER, "bev"),
    "vamp_render_indices": (RENDER, None), "vamp_render_camera_direct_taps": (RENDER, None),
    "vamp_frustum_geometry": (RENDER, None),
    "vamp_sample_points_forward": (SAMPLE, None), "vamp_sample_points_backward": (SAMPLE, "sample"),
    "vamp_depth_softmax_forward": (SOFTMAX, None), "vamp_depth_softmax_backward": (SOFTMAX, None),
    "vamp_density_gate_forward": (GATE, None), "vamp_density_gate_backward": (GATE, None),
    "vamp_gate_conv1x1_forward": (GATE_CONV, None), "vamp_gate_conv1x1_backward": (GATE_CONV, "gate_conv"),
}

_PROTOS = header_prototypes()


def _is_pointer(ctype):
    return ctype.endswith("*")


def _table():
    """{(function, parameter): ("tensor", shape, dtype source, alignment) | ("workspace", size parameter, bytes)} for
    every pointer parameter of the covered functions that can carry a tensor."""
    table = {}
    for fn, (family, ws) in FUNCTIONS.items():
        for ctype, name in _PROTOS.get(fn, ()):
            if not _is_pointer(ctype) or name in EXCLUDED:
                continue
            if ws is not None and name in WORKSPACE[ws]:
                table[(fn, name)] = ("workspace",) + WORKSPACE[ws][name]
            elif name in family:
                table[(fn, name)] = ("tensor",) + family[name]
    return table


TABLE = _table()


class CallGuard:
    """`vamp` (HotPath.vamp, or a stand-in with the same attributes) behind the checks; `log` holds (function,
    arguments) of every guarded call that was FORWARDED.  `device`: where every tensor has to live; `sizes`: the object
    asked for the `*_workspace_bytes` (the checked library by default); `alignment` False leaves the alignment
    requirements to the library, which checks them on the host itself (to see ITS message)."""

    def __init__(self, vamp, device, sizes=None, alignment=True):
        self._vamp, self._sizes, self._alignment, self.log = vamp, sizes, alignment, []
        self.device = torch.device(device)

    def _query(self):
        return self._sizes if self._sizes is not None else _capi.checked()

    def __getattr__(self, name):
        fn = getattr(self._vamp, name)
        if name not in FUNCTIONS:
            return fn

        def call(*args):
            self.check(name, args)
            self.log.append((name, args))
            return fn(*args)
        return call

    # ------------------------------------------------------------------ the checks
    def check(self, name, args):
        proto = _PROTOS[name]
        if len(args) != len(proto):
            raise ContractViolation(name, "*", f"{len(args)} arguments for {len(proto)} parameters")
        a = types.SimpleNamespace(function=name, **{p: v for (_, p), v in zip(proto, args)})
        for (ctype, pname), v in zip(proto, args):
            if not isinstance(v, torch.Tensor):
                continue
            spec = TABLE.get((name, pname))
            if spec is None:
                raise ContractViolation(name, pname, "a tensor in a parameter the table does not know")
            self._device(name, pname, v)
            if spec[0] == "workspace":
                self._workspace(name, pname, v, a, spec[1], spec[2])
            else:
                self._tensor(name, pname, ctype, v, a, *spec[1:])

    def _device(self, name, pname, t):
        want = self.device
        if t.device.type != want.type or (want.index is not None and t.device.index != want.index):
            raise ContractViolation(name, pname, f"device: a tensor on {t.device}, the call runs on {want}")

    def _workspace(self, name, pname, t, a, size_param, need):
        if not t.is_contiguous():
            raise ContractViolation(name, pname, f"layout: not contiguous (strides {t.stride()})")
        have, said, want = t.numel() * t.element_size(), int(getattr(a, size_param)), int(need(self._query(), a))
        if said > have:
            raise ContractViolation(name, pname, f"size: {size_param} = {said} for a buffer of {have} bytes")
        if said < want:
            raise ContractViolation(name, pname, f"size: {said} bytes, the call needs {want}")

    def _tensor(self, name, pname, ctype, t, a, shape, dtype_src, align):
        shape = tuple(int(s) for s in shape(a))
        flag, which = CHANNEL_LAST.get(name, (0, ()))
        if pname in which and (a.flags & flag):
            # the one declared exception: [B, N, C, fH, fW] values in [B, N, fH, fW, C] memory, 16-byte aligned
            if t.dim() != 5 or not t.permute(0, 1, 3, 4, 2).is_contiguous():
                raise ContractViolation(name, pname, f"layout: not channel-last (shape {tuple(t.shape)}, strides {t.stride()})")
            align = 16
        elif not t.is_contiguous():
            raise ContractViolation(name, pname, f"layout: not contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
        if t.numel() != math.prod(shape):
            raise ContractViolation(name, pname, f"size: {t.numel()} elements {tuple(t.shape)}, the descriptor implies "
                                                 f"{math.prod(shape)} {shape}")
        base = ctype.replace("const ", "").rstrip("*").strip()
        if base == "void":
            code = _desc(a.d).in_dtype if dtype_src == DESC else getattr(a, dtype_src)
            want = DTYPE_BYTES.get(int(code))
            if want is None:
                raise ContractViolation(name, pname, f"dtype: code {code} names no dtype of the hot path")
            if not t.is_floating_point():
                raise ContractViolation(name, pname, f"dtype: {t.dtype} where code {code} travels")
        else:
            want = ELEMENT_BYTES[base]
            if base == "float" and t.dtype != torch.float32:
                raise ContractViolation(name, pname, f"dtype: {t.dtype} for a float* parameter")
        if t.element_size() != want:
            raise ContractViolation(name, pname, f"dtype: {t.dtype} ({t.element_size()} bytes per element), the call reads "
                                                 f"{want}")
        if self._alignment and align and t.data_ptr() % align:
            raise ContractViolation(name, pname, f"alignment: address {t.data_ptr():#x} is not a multiple of {align}")


def install(hp, **kw):
    """Put `hp`'s library calls behind the guard; returns it (its `log` is the record of what was forwarded)."""
    guard = CallGuard(hp.vamp, hp.device, **kw)
    hp.vamp = guard
    return guard
