"""Camera images on the device (Python over the C ABI): the image half of the reference loader's camera path,
img_transform (nusc_det_seg_dataset.py:118-146: Pillow's resize, crop, flip, rotate) followed by mmcv.imnormalize
(:679-681), with the augmentation values of sample_ida_augmentation (:472-499) that `labels.ida_table` takes too.
`plan_camera_images` does the float64 work on the host (bicubic taps, rotation constants: rules 1 and 4 of
include/vampire_hip.h) and touches no GPU; `camera_images` runs the two HIP kernels of vamp_camera_images on the
plan's int32 tables in device memory.  There is no CPU fallback.

Rules 1 - 4 are pinned byte for byte against Pillow 12.2.0 (tests/golden/camera_images.npz; the reference does not
pin Pillow).  The normalisation restates mmcv.imnormalize -- (float32(img) - mean) * float32(1 / float64(std)) after
OpenCV's BGR -> RGB swap applied to Pillow's RGB image -- and its parity with OpenCV is UNPINNED: neither OpenCV nor
mmcv was available to compare against."""
import dataclasses
import functools
import math

import numpy as np
import torch

from . import _capi
from ._tensors import DTYPE_CODES, _stream, check_out, need_device, scratch, workspace_bytes

IMG_MEAN, IMG_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)      # the reference's img_conf
_TABLES = ("col_first", "col_count", "col_taps", "row_first", "row_count", "row_taps", "consts")
_K, _TW, _TH = _capi.VAMP_IMG_MAX_TAPS, _capi.VAMP_IMG_TILE_W, _capi.VAMP_IMG_TILE_H
_OUT_DTYPES = (torch.float32, torch.bfloat16)


def _cubic(x):
    x = np.abs(x)
    return np.where(x < 1.0, ((1.5 * x - 2.5) * x) * x + 1.0,
                    np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * -0.5, 0.0))


@functools.lru_cache(maxsize=256)
def _axis_taps(n_in, n_out):
    """Rule 1 for one axis: (first [n_out], count [n_out], taps [n_out, max count]) as int64 / int32 arrays, the
    taps zero behind their count."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = 2.0 * fs, 1.0 / fs
    c = (np.arange(n_out) + 0.5) * scale
    lo = np.maximum((c - support + 0.5).astype(np.int64), 0)           # astype truncates, as the C cast does
    hi = np.minimum((c + support + 0.5).astype(np.int64), n_in)
    cnt = hi - lo
    j = np.arange(int(cnt.max()))
    live = j[None] < cnt[:, None]
    k = np.where(live, _cubic(((j[None] + lo[:, None]) - c[:, None] + 0.5) * ss), 0.0)
    ww = np.cumsum(k, axis=1)[:, -1:]                                   # summed from left to right
    k = np.where(ww != 0.0, k / np.where(ww != 0.0, ww, 1.0), k)
    ki = np.where(k < 0.0, np.trunc(k * 4194304.0 - 0.5), np.trunc(k * 4194304.0 + 0.5)).astype(np.int32)
    return lo, cnt, np.where(live, ki, 0).astype(np.int32)


def _axis_foot(first, cnt, tile):
    """The widest raw span under `tile` consecutive outputs of an axis, wherever the tile starts."""
    n = len(first)
    if n == 0:
        return 0
    end = first + cnt
    return int(max((end[i:i + tile].max() - first[i:i + tile].min()) for i in range(max(n - tile + 1, 1))))


def _rotate_consts(rotate, W, H):
    """Rule 4: a0 .. a5."""
    a = -math.radians(rotate % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = (m[0] * -cx + m[1] * -cy + m[2]) + cx
    m[5] = (m[3] * -cx + m[4] * -cy + m[5]) + cy
    fix = lambda v: math.floor(v * 65536.0 + 0.5)
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]),
            fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def _window(n_in, n_new, start, n, what):
    """The tables of the `n` resized outputs start .. start + n - 1 of an axis resized n_in -> n_new: first, count,
    taps [K, n] (tap-major), and the largest raw span under one tile."""
    if n_new < 1:
        raise ValueError(f"resize_dims: the resized {what} {n_new} must be positive")
    lo, cnt, ki = _axis_taps(int(n_in), int(n_new))
    if ki.shape[1] > _K:
        raise ValueError(f"resizing {what} {n_in} -> {n_new} needs {ki.shape[1]} taps per output, the library holds "
                         f"{_K}: the resize is outside its range (about 0.27 and above)")
    at = start + np.arange(n)
    inside = (at >= 0) & (at < n_new)
    src = np.clip(at, 0, n_new - 1)
    first = np.where(inside, lo[src], 0)
    count = np.where(inside, cnt[src], 0)
    taps = np.zeros((_K, n), np.int32)
    taps[:ki.shape[1]] = np.where(inside[None], ki[src].T, 0)
    live = count > 0
    foot = 0
    for t0 in range(0, n, _TW if what == "width" else _TH):
        sl = slice(t0, t0 + (_TW if what == "width" else _TH))
        if live[sl].any():
            foot = max(foot, int((first[sl] + count[sl])[live[sl]].max() - first[sl][live[sl]].min()))
    return first.astype(np.int32), count.astype(np.int32), taps, foot


def _tables(augs, raw_dim, final_dim):
    raw_h, raw_w = (int(v) for v in raw_dim)
    H, W = (int(v) for v in final_dim)
    if not augs or not augs[0] or len({len(r) for r in augs}) != 1:
        raise ValueError("augs must be a [B][N] nesting of (resize, resize_dims, crop, flip, rotate) tuples")
    B, N = len(augs), len(augs[0])
    t = dict(col_first=np.zeros((B, N, W), np.int32), col_count=np.zeros((B, N, W), np.int32),
             col_taps=np.zeros((B, N, _K, W), np.int32), row_first=np.zeros((B, N, H), np.int32),
             row_count=np.zeros((B, N, H), np.int32), row_taps=np.zeros((B, N, _K, H), np.int32),
             consts=np.zeros((B, N, _capi.VAMP_IMG_CONST_COLS), np.int32))
    foot_w = foot_h = 1
    for b, per_sample in enumerate(augs):
        for n, (_resize, resize_dims, crop, flip, rotate) in enumerate(per_sample):
            new_w, new_h = (int(v) for v in resize_dims)
            x0, y0 = int(crop[0]), int(crop[1])
            if tuple(crop) != (x0, y0, x0 + W, y0 + H):
                raise ValueError(f"augs[{b}][{n}]: crop {tuple(crop)} is not an integer {W} x {H} window (final_dim)")
            if not abs(rotate) < 45:
                raise ValueError(f"augs[{b}][{n}]: rotate {rotate} must be within (-45, 45) degrees")
            t["col_first"][b, n], t["col_count"][b, n], t["col_taps"][b, n], fw = _window(raw_w, new_w, x0, W, "width")
            t["row_first"][b, n], t["row_count"][b, n], t["row_taps"][b, n], fh = _window(raw_h, new_h, y0, H, "height")
            foot_w, foot_h = max(foot_w, fw), max(foot_h, fh)
            t["consts"][b, n, :11] = _rotate_consts(float(rotate), W, H) + [x0, y0, new_w, new_h, 1 if flip else 0]
    if foot_w > _capi.VAMP_IMG_FOOT_W or foot_h > _capi.VAMP_IMG_FOOT_H:
        raise ValueError(f"a tile's raw footprint {foot_h} x {foot_w} exceeds the library's {_capi.VAMP_IMG_FOOT_H} x "
                         f"{_capi.VAMP_IMG_FOOT_W}: the resize is outside its range")
    return t, (B, N, raw_h, raw_w, H, W), foot_w, foot_h


@dataclasses.dataclass
class ImagePlan:
    """The int32 plan tables of `camera_images` (include/vampire_hip.h, vamp_camera_images) as numpy arrays, and after
    `to(device)` as views of ONE device buffer that `update` refills in place.  foot_w, foot_h: the largest raw
    footprint under one tile this plan may ever need; they size the resample kernel's LDS and are fixed for the
    plan's life (a captured graph keeps them)."""
    B: int
    N: int
    raw_dim: tuple
    final_dim: tuple
    foot_w: int
    foot_h: int
    col_first: np.ndarray
    col_count: np.ndarray
    col_taps: np.ndarray
    row_first: np.ndarray
    row_count: np.ndarray
    row_taps: np.ndarray
    consts: np.ndarray
    device_tables: dict = None      # name -> int32 device view, after to()
    _flat: torch.Tensor = None

    def _pack(self):
        return torch.from_numpy(np.concatenate([getattr(self, k).ravel() for k in _TABLES]))

    def to(self, device):
        """The tables in one int32 buffer on `device`; returns self."""
        self._flat = self._pack().to(device)
        self.device_tables, at = {}, 0
        for k in _TABLES:
            a = getattr(self, k)
            self.device_tables[k] = self._flat[at:at + a.size].view(a.shape)
            at += a.size
        return self

    def update(self, augs):
        """New augmentation values for the same shapes: the numpy tables are replaced and the SAME device buffer is
        refilled with one copy_, so a captured graph replays with the new values.  Raises when the new values need a
        larger footprint than the plan was made for (see `plan_camera_images`, resize_min)."""
        t, dims, foot_w, foot_h = _tables(augs, self.raw_dim, self.final_dim)
        if dims[:2] != (self.B, self.N):
            raise ValueError(f"augs is {dims[0]} x {dims[1]}, the plan {self.B} x {self.N}")
        if foot_w > self.foot_w or foot_h > self.foot_h:
            raise ValueError(f"the new values need a raw footprint of {foot_h} x {foot_w} under a tile, the plan was "
                             f"made for {self.foot_h} x {self.foot_w}: give plan_camera_images a resize_min")
        for k in _TABLES:
            setattr(self, k, t[k])
        if self._flat is not None:
            self._flat.copy_(self._pack())
        return self


def plan_camera_images(augs, raw_dim, final_dim, resize_min=None):
    """The ImagePlan of `augs[b][n]`, the (resize, resize_dims, crop, flip, rotate) tuples of sample_ida_augmentation
    that `labels.ida_table` takes, for raw frames raw_dim = (raw_h, raw_w) and final_dim = (H, W).  Pure host work in
    float64 (rules 1 and 4 of include/vampire_hip.h); no GPU is touched.  resize_min: the smallest resize a later
    `update` may bring (the reference's resize_lim[0]); the plan's footprint capacity is then sized for it.
    Raises ValueError on |rotate| >= 45 (Pillow switches to transposes at multiples of 90), on a crop that is not a
    final_dim window, and on a resize outside the library's range (more than 16 taps per output: below about 0.27)."""
    t, (B, N, raw_h, raw_w, H, W), foot_w, foot_h = _tables(augs, raw_dim, final_dim)
    if resize_min is not None:
        for n_in, tile, cap, name in ((raw_w, _TW, _capi.VAMP_IMG_FOOT_W, "w"), (raw_h, _TH, _capi.VAMP_IMG_FOOT_H, "h")):
            n_new = int(n_in * resize_min)
            if n_new < 1:
                raise ValueError(f"resize_min {resize_min} leaves no pixel of {n_in}")
            lo, cnt, ki = _axis_taps(n_in, n_new)
            if ki.shape[1] > _K:
                raise ValueError(f"resize_min {resize_min} needs {ki.shape[1]} taps per output, the library holds {_K}")
            foot = min(_axis_foot(lo, cnt, tile) + 2, cap)              # (+ 2: int() of the resized size in between)
            if name == "w":
                foot_w = max(foot_w, foot)
            else:
                foot_h = max(foot_h, foot)
    return ImagePlan(B=B, N=N, raw_dim=(raw_h, raw_w), final_dim=(H, W), foot_w=foot_w, foot_h=foot_h, **t)


def camera_images(raw, plan, *, mean=IMG_MEAN, std=IMG_STD, to_rgb=True, dtype=torch.float32, out=None, out_u8=None):
    """Resize, crop, flip, rotate and normalise raw camera frames as the reference loader does (vamp_camera_images),
    in two launches on the current stream, without a host synchronisation; capturable in a graph, and a replay
    follows `plan.update`.

    raw: [B, N, raw_h, raw_w, 3] uint8 on the device (Pillow's RGB order), dense along its last two axes; any batch,
    camera and row stride and any alignment are read in place (a slice of a wider or taller buffer).  plan: an
    ImagePlan after `to(device)`.  mean, std: three numbers each; to_rgb: the channel swap of mmcv.imnormalize.
    dtype: torch.float32 or torch.bfloat16 (round-to-nearest-even of the fp32 value), or None for the uint8 image
    alone.  out: a [B, N, 3, H, W] tensor of an earlier call to write again; out_u8: True, or a [B, N, H, W, 3] uint8
    tensor to write again, to get the transformed uint8 image (rule 4's) as well.
    Returns the normalised [B, N, 3, H, W] tensor, or (normalised | None, uint8 image) when out_u8 is asked for.
    The parity of the normalisation with OpenCV is unpinned (module docstring)."""
    need_device("camera_images", raw)
    if plan.device_tables is None:
        raise ValueError("the plan's tables are on the host: call plan.to(device) first")
    need_device("camera_images", plan._flat)
    if raw.dtype != torch.uint8:
        raise TypeError(f"raw must be uint8, got {raw.dtype}")
    raw_h, raw_w = plan.raw_dim
    H, W = plan.final_dim
    B, N = plan.B, plan.N
    if tuple(raw.shape) != (B, N, raw_h, raw_w, 3):
        raise ValueError(f"raw: expected {(B, N, raw_h, raw_w, 3)}, got {tuple(raw.shape)}")
    if raw.stride(4) != 1 or raw.stride(3) != 3:
        raise ValueError(f"raw must be dense along its last two axes (strides (3, 1)), got {tuple(raw.stride()[3:])}: "
                         "pixels are read as three interleaved bytes")
    sb, sn, sr = raw.stride(0), raw.stride(1), raw.stride(2)
    if (raw_h > 1 and sr < 3 * raw_w) or min(sb, sn, sr) < 0:
        raise ValueError(f"raw: rows overlap (strides {tuple(raw.stride())})")
    dev = raw.device
    if plan._flat.device != dev:
        raise ValueError(f"the plan is on {plan._flat.device}, raw on {dev}")
    if dtype is not None and dtype not in _OUT_DTYPES:
        raise TypeError(f"dtype must be torch.float32, torch.bfloat16 or None, got {dtype}")
    want_u8 = out_u8 is not None and out_u8 is not False
    if dtype is None and not want_u8:
        raise ValueError("nothing to do: dtype is None and out_u8 is not asked for")
    if dtype is None and out is not None:
        raise ValueError("out belongs to a dtype")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std take three numbers each")

    d = _capi.VampImageDesc()
    d.raw_b_stride, d.raw_n_stride, d.raw_row_stride = sb, sn, max(sr, 3 * raw_w)
    d.B, d.N, d.raw_h, d.raw_w, d.H, d.W = B, N, raw_h, raw_w, H, W
    d.taps_x = d.taps_y = _K
    d.foot_w, d.foot_h = plan.foot_w, plan.foot_h
    d.out_dtype = _capi.VAMP_IMG_OUT_NONE if dtype is None else DTYPE_CODES[dtype]
    d.to_rgb = 1 if to_rgb else 0
    for c in range(3):
        d.mean[c] = float(np.float32(mean[c]))
        d.std_inv[c] = float(np.float32(1.0 / np.float64(std[c])))

    vamp = _capi.checked()
    nbytes = workspace_bytes(vamp.vamp_camera_images_workspace_bytes, d,
                             lambda: vamp.vamp_camera_images(d, *([None] * 11), 0, None))
    if dtype is not None:
        out = (torch.empty(B, N, 3, H, W, dtype=dtype, device=dev) if out is None
               else check_out(out, (B, N, 3, H, W), dtype, dev, "out", align=16))
    if want_u8:
        out_u8 = (torch.empty(B, N, H, W, 3, dtype=torch.uint8, device=dev) if out_u8 is True
                  else check_out(out_u8, (B, N, H, W, 3), torch.uint8, dev, "out_u8", align=16))
    t = plan.device_tables
    with torch.cuda.device(dev):
        ws = scratch("camera_images", dev, nbytes)
        vamp.vamp_camera_images(d, raw, *(t[k] for k in _TABLES), out, out_u8 if want_u8 else None, ws, ws.numel(),
                                _stream())
    return (out, out_u8) if want_u8 else out


def ida_mats(augs):
    """The fp32 [B, N, 4, 4] post-homography matrices of img_transform (nusc_det_seg_dataset.py:128-145) for
    `augs[b][n]`, with the same torch fp32 operations in the same order (the rotation's cos / sin are taken in
    float64 and rounded to fp32 when the 2 x 2 is made, as get_rot does), on the host."""
    if not augs or not augs[0] or len({len(r) for r in augs}) != 1:
        raise ValueError("augs must be a [B][N] nesting of (resize, resize_dims, crop, flip, rotate) tuples")
    rows = []
    for per_sample in augs:
        row = []
        for resize, _resize_dims, crop, flip, rotate in per_sample:
            rot = torch.eye(2) * resize
            tran = torch.zeros(2) - torch.Tensor(crop[:2])
            if flip:
                A = torch.Tensor([[-1, 0], [0, 1]])
                rot = A.matmul(rot)
                tran = A.matmul(tran) + torch.Tensor([crop[2] - crop[0], 0])
            h = rotate / 180 * np.pi
            A = torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
            b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
            b = A.matmul(-b) + b
            mat = torch.zeros(4, 4)
            mat[2, 2] = mat[3, 3] = 1
            mat[:2, :2] = A.matmul(rot)
            mat[:2, 3] = A.matmul(tran) + b
            row.append(mat)
        rows.append(torch.stack(row))
    return torch.stack(rows)


def fill_train_images(batch, raw, augs, cfg, *, mean=IMG_MEAN, std=IMG_STD, to_rgb=True, plan=None):
    """A copy of a collate_fn(mode='train')-shaped batch (multitask.synthetic_batch) whose entry 0 -- sweep_imgs
    [B, 1, N, 3, H, W] fp32 -- is `camera_images` of the raw frames `raw` [B, N, raw_h, raw_w, 3] uint8 under `augs`
    (see `labels.ida_table`), and whose ida_mats (entry 1) are `ida_mats(augs)`: the sibling of
    `labels.fill_train_labels`, so that images, matrices and labels agree on one set of augmentation values.
    cfg: the PathConfig (final_dim); plan: an ImagePlan on raw's device to use (and update) instead of a new one."""
    if plan is None:
        plan = plan_camera_images(augs, tuple(raw.shape[2:4]), cfg.final_dim).to(raw.device)
    else:
        plan.update(augs)
    imgs = camera_images(raw, plan, mean=mean, std=std, to_rgb=to_rgb)
    new = list(batch)
    new[0] = imgs[:, None]
    mats = dict(batch[1])
    mats["ida_mats"] = ida_mats(augs)[:, None].to(raw.device)
    new[1] = mats
    return new
