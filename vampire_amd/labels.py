"""Training labels rasterised from the lidar points on the device (Python over the C ABI): the camera depth /
segmentation maps of the reference loader's depth_transform (nusc_det_seg_dataset.py:178-231, behind the margins of
map_pointcloud_to_image, :362-367), the BEV segmentation / height / mask maps of get_bev_seg_map (:233-265) and the
every-s-th-pixel pick of get_downsampled_gt (base_exp.py:596-632).  All work happens in hand-written HIP kernels
reached through `_capi` (vamp_lidar_labels: fill, scatter with 64-bit integer atomic min / max, resolve); there is no
CPU fallback."""
import dataclasses

import numpy as np
import torch

from . import _capi
from ._tensors import (DTYPE_CODES, _aligned, _pad_samples, _stream, check_out, list_dtype, need_device, scratch,
                       workspace_bytes)

_LABEL_DTYPES = (torch.uint8, torch.int64)


@dataclasses.dataclass
class LidarLabels:
    """What `lidar_labels` returns; the fields of a part that was not asked for are None.  cam_fg and bev_mask are
    bool views of the uint8 buffers the kernels write."""
    cam_depth: torch.Tensor = None     # [B, N, h, w] fp32, 0 where no point landed
    cam_seg: torch.Tensor = None       # [B, N, h, w] int64
    cam_fg: torch.Tensor = None        # [B, N, h, w] bool: cam_depth > 0
    bev_seg: torch.Tensor = None       # [B, 1, 1, ny, nx] int64, as collate_fn stacks it
    bev_height: torch.Tensor = None    # [B, 1, 1, ny, nx] fp32, 0 where empty
    bev_mask: torch.Tensor = None      # [B, 1, 1, ny, nx] bool


def _pack_points(points, labels, counts):
    """Per-sample lists ([n_b, 3 | 4] points, [n_b] labels) -> padded [B, M, 3 | 4], [B, M] and int32 counts [B] on
    the device.  The counts come from the shapes, one scalar fill per sample: nothing is read back from the device
    and nothing is copied to it.  Packed tensors pass through."""
    if isinstance(points, torch.Tensor):
        if not isinstance(labels, torch.Tensor):
            raise ValueError("points is a packed tensor but labels is not")
        return points, labels, counts
    if counts is not None:
        raise ValueError("counts belongs to packed points: per-sample lists carry their own lengths")
    if len(points) != len(labels) or len(points) == 0:
        raise ValueError(f"{len(points)} point tensors and {len(labels)} label tensors (one per sample, at least one)")
    need_device("lidar_labels", list(points), list(labels))
    list_dtype(points, "points", torch.float32, "fp32")
    list_dtype(labels, "labels")
    if any(p.dim() != 2 or l.dim() != 1 or p.shape[0] != l.shape[0] for p, l in zip(points, labels)):
        raise ValueError("every sample needs points [n, 3 | 4] and labels [n]")
    if len({p.shape[1] for p in points}) != 1:
        raise ValueError("the samples' points must share one column count")
    return _pad_samples(points, labels)


def _bev_grid(bev):
    """(ny, nx, origin_x, origin_y, size, z_lo, z_hi) of a `bev` dict, the cell counts as get_bev_seg_map computes
    them: int((hi - lo) / size)."""
    unknown = set(bev) - {"x_bound", "y_bound", "z_bound", "size"}
    if unknown or "x_bound" not in bev or "y_bound" not in bev:
        raise ValueError(f"bev takes x_bound, y_bound and optionally z_bound, size; got {sorted(bev)}")
    xb, yb = bev["x_bound"], bev["y_bound"]
    zb, size = bev.get("z_bound", (-5., 3.)), float(bev.get("size", 0.4))
    if not size > 0:
        raise ValueError(f"bev size must be positive, got {size}")
    nx, ny = int((xb[1] - xb[0]) / size), int((yb[1] - yb[0]) / size)
    return ny, nx, xb[0] - size / 2.0, yb[0] - size / 2.0, size, float(zb[0]), float(zb[1])


def lidar_labels(points, labels, *, lidar2cam=None, intrins=None, aug=None, final_dim=None, raw_dim=None, stride=1,
                 bev=None, counts=None, out=None):
    """Rasterise lidar points into camera depth / segmentation labels and BEV segmentation / height / mask labels
    (vamp_lidar_labels) in three launches on the current stream, without a host synchronisation; with packed inputs
    the call can be captured in a graph.

    points, labels: per-sample lists ([n_b, 3 | 4] fp32 in the bda-augmented ego frame, [n_b] uint8 | int64), padded
    here with the counts taken from the shapes, or packed [B, M, 3 | 4] and [B, M] tensors with `counts` (int32 [B]
    on the device; None: all M rows count).
    Camera part (when lidar2cam is given): lidar2cam, intrins [B, N, 4, 4] fp32, aug [B, N, 8] float64 on the device
    (`ida_table`), final_dim (H, W), raw_dim (raw_h, raw_w) of the image the intrinsics belong to, stride s: the
    labels are map[::s, ::s] of the full-resolution maps.  The nearest point wins a pixel; equal depths go to the
    lowest point index (the reference's order there is undefined).
    BEV part (when bev is given): dict(x_bound, y_bound, z_bound=(-5., 3.), size=0.4), bounds as (lo, hi[, ...]);
    the highest point wins a cell, equal heights go to the lowest index.
    out: a LidarLabels of an earlier call with the same shapes, whose buffers are written again.
    Returns a LidarLabels."""
    points, labels, counts = _pack_points(points, labels, counts)
    need_device("lidar_labels", points, labels)
    if points.dtype != torch.float32:
        raise TypeError(f"points must be fp32, got {points.dtype}")
    if labels.dtype not in _LABEL_DTYPES:
        raise TypeError(f"labels must be uint8 or int64, got {labels.dtype}")
    if points.dim() != 3 or points.shape[2] not in (3, 4) or tuple(labels.shape) != tuple(points.shape[:2]):
        raise ValueError(f"expected points [B, M, 3 | 4] and labels [B, M], got {tuple(points.shape)} "
                         f"and {tuple(labels.shape)}")
    B, M, cols = points.shape
    dev = points.device
    if counts is not None:
        need_device("lidar_labels", counts)
        if counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
            raise ValueError(f"counts must be int32 [{B}], got {counts.dtype} {tuple(counts.shape)}")
        counts = _aligned(counts)
    cam, do_bev = lidar2cam is not None, bev is not None
    if not cam and not do_bev:
        raise ValueError("nothing to do: give lidar2cam (with intrins, aug, final_dim, raw_dim) and / or bev")
    if not cam and not (intrins is None and aug is None and final_dim is None and raw_dim is None):
        raise ValueError("intrins, aug, final_dim and raw_dim belong to the camera part: lidar2cam is missing")

    d = _capi.VampLidarLabelDesc()
    d.B, d.M, d.point_cols, d.label_dtype = B, M, cols, DTYPE_CODES[labels.dtype]
    # the part that is not asked for: the smallest valid grid (the library checks the whole descriptor)
    d.N, d.H, d.W, d.stride, d.raw_w, d.raw_h = 1, 1, 1, 1, 1, 1
    d.ny, d.nx, d.size, d.z_lo, d.z_hi = 1, 1, 1.0, -1.0, 1.0
    if cam:
        if intrins is None or aug is None or final_dim is None or raw_dim is None:
            raise ValueError("the camera part needs lidar2cam, intrins, aug, final_dim and raw_dim")
        need_device("lidar_labels", lidar2cam, intrins, aug)
        if lidar2cam.dim() != 4 or tuple(lidar2cam.shape[2:]) != (4, 4) or lidar2cam.shape[0] != B:
            raise ValueError(f"lidar2cam: expected [{B}, N, 4, 4], got {tuple(lidar2cam.shape)}")
        N = lidar2cam.shape[1]
        if tuple(intrins.shape) != (B, N, 4, 4):
            raise ValueError(f"intrins: expected {(B, N, 4, 4)}, got {tuple(intrins.shape)}")
        if tuple(aug.shape) != (B, N, 8):
            raise ValueError(f"aug: expected {(B, N, 8)}, got {tuple(aug.shape)}")
        if lidar2cam.dtype != torch.float32 or intrins.dtype != torch.float32:
            raise TypeError(f"lidar2cam and intrins must be fp32, got {lidar2cam.dtype} and {intrins.dtype}")
        if aug.dtype != torch.float64:
            raise TypeError(f"aug must be float64 (ida_table), got {aug.dtype}")
        H, W = (int(v) for v in final_dim)
        raw_h, raw_w = (int(v) for v in raw_dim)
        stride = int(stride)
        if stride < 1 or H % stride or W % stride:
            raise ValueError(f"stride {stride} must be positive and divide final_dim {(H, W)}")
        d.N, d.H, d.W, d.stride, d.raw_w, d.raw_h = N, H, W, stride, raw_w, raw_h
        lidar2cam, intrins, aug = _aligned(lidar2cam), _aligned(intrins), _aligned(aug)
        h, w = H // stride, W // stride
    if do_bev:
        ny, nx, ox, oy, size, z_lo, z_hi = _bev_grid(bev)
        d.ny, d.nx, d.origin_x, d.origin_y, d.size, d.z_lo, d.z_hi = ny, nx, ox, oy, size, z_lo, z_hi

    vamp = _capi.checked()
    nbytes = workspace_bytes(vamp.vamp_lidar_labels_workspace_bytes, d,
                             lambda: vamp.vamp_lidar_labels(d, *([None] * 13), 0, None))
    points, labels = _aligned(points), _aligned(labels)
    if out is None:
        out = LidarLabels()
        if cam:
            out.cam_depth = torch.empty(B, N, h, w, dtype=torch.float32, device=dev)
            out.cam_seg = torch.empty(B, N, h, w, dtype=torch.int64, device=dev)
            out.cam_fg = torch.empty(B, N, h, w, dtype=torch.uint8, device=dev).view(torch.bool)
        if do_bev:
            out.bev_seg = torch.empty(B, 1, 1, ny, nx, dtype=torch.int64, device=dev)
            out.bev_height = torch.empty(B, 1, 1, ny, nx, dtype=torch.float32, device=dev)
            out.bev_mask = torch.empty(B, 1, 1, ny, nx, dtype=torch.uint8, device=dev).view(torch.bool)
    else:
        if cam:
            check_out(out.cam_depth, (B, N, h, w), torch.float32, dev, "out.cam_depth")
            check_out(out.cam_seg, (B, N, h, w), torch.int64, dev, "out.cam_seg")
            check_out(out.cam_fg, (B, N, h, w), torch.bool, dev, "out.cam_fg")
        if do_bev:
            check_out(out.bev_seg, (B, 1, 1, ny, nx), torch.int64, dev, "out.bev_seg")
            check_out(out.bev_height, (B, 1, 1, ny, nx), torch.float32, dev, "out.bev_height")
            check_out(out.bev_mask, (B, 1, 1, ny, nx), torch.bool, dev, "out.bev_mask")
    u8 = lambda t: t.view(torch.uint8)
    cam_args = (out.cam_depth, out.cam_seg, u8(out.cam_fg)) if cam else (None, None, None)
    bev_args = (out.bev_seg, out.bev_height, u8(out.bev_mask)) if do_bev else (None, None, None)
    with torch.cuda.device(dev):
        ws = scratch("lidar_labels", dev, nbytes)
        vamp.vamp_lidar_labels(d, points, labels, counts, lidar2cam if cam else None, intrins if cam else None,
                               aug if cam else None, *cam_args, *bev_args, ws, ws.numel(), _stream())
    return out


def ida_table(augs, device):
    """The float64 [B, N, 8] augmentation table of `lidar_labels` (resize, crop_x, crop_y, flip, cos, sin, 0, 0) from
    `augs[b][n]`, the (resize, resize_dims, crop, flip, rotate) tuples of sample_ida_augmentation
    (nusc_det_seg_dataset.py:472-499); cos / sin of rotate / 180 * pi in float64, as depth_transform takes them."""
    rows = []
    for per_sample in augs:
        row = []
        for resize, _resize_dims, crop, flip, rotate in per_sample:
            h = rotate / 180 * np.pi
            row.append([float(resize), float(crop[0]), float(crop[1]), 1.0 if flip else 0.0, float(np.cos(h)),
                        float(np.sin(h)), 0.0, 0.0])
        rows.append(row)
    if not rows or not rows[0] or len({len(r) for r in rows}) != 1:
        raise ValueError("augs must be a [B][N] nesting of (resize, resize_dims, crop, flip, rotate) tuples")
    return torch.tensor(rows, dtype=torch.float64).to(device)


def lidar2cam_from_mats(mats):
    """lidar2cam [B, N, 4, 4] fp32 for `lidar_labels` from a batch's matrix dict: inv(sensor2ego) . inv(bda), taken
    in float64 on the host -- points in the bda-augmented ego frame go back to the ego frame and on into each
    camera.  This is the composition for points and cameras that share a timestamp (the synthetic batches); a sweep
    taken at another time needs the ego-motion between the two in the middle."""
    s2e, bda = mats["sensor2ego_mats"], mats["bda_mat"]
    if s2e.dim() == 5:                                   # [B, sweeps, N, 4, 4]: the key frame
        s2e = s2e[:, 0]
    if s2e.dim() != 4 or tuple(s2e.shape[2:]) != (4, 4) or tuple(bda.shape) != (s2e.shape[0], 4, 4):
        raise ValueError(f"expected sensor2ego_mats [B, (1,) N, 4, 4] and bda_mat [B, 4, 4], got {tuple(s2e.shape)} "
                         f"and {tuple(bda.shape)}")
    out = torch.linalg.inv(s2e.detach().double().cpu()) @ torch.linalg.inv(bda.detach().double().cpu())[:, None]
    return out.float().to(s2e.device)


def fill_train_labels(batch, cfg, augs, stride=1, raw_dim=(900, 1600)):
    """A copy of a collate_fn(mode='train')-shaped batch (multitask.synthetic_batch) whose entries 6 - 10 -- camera
    depth / segmentation labels, BEV segmentation / height / mask -- are the rasterised labels of its own points
    (entry 11), point labels (entry 12) and matrices (entry 1), so that the labels agree with the batch's geometry.
    cfg: the PathConfig (final_dim, the BEV grid of x_bound_det / y_bound_det); augs: see `ida_table`; raw_dim:
    (raw_h, raw_w) of the images the intrinsics belong to.  With stride 1 the shapes are those of the entries
    replaced."""
    mats, pts, lab = batch[1], batch[11], batch[12]
    dev = pts[0].device
    intr = mats["intrin_mats"]
    intr = (intr[:, 0] if intr.dim() == 5 else intr).float().to(dev)
    bev = dict(x_bound=tuple(cfg.x_bound_det[:2]), y_bound=tuple(cfg.y_bound_det[:2]), z_bound=(-5., 3.),
               size=cfg.x_bound_det[2])
    got = lidar_labels(pts, lab, lidar2cam=lidar2cam_from_mats(mats).to(dev), intrins=intr, aug=ida_table(augs, dev),
                       final_dim=cfg.final_dim, raw_dim=raw_dim, stride=stride, bev=bev)
    new = list(batch)
    new[6], new[7] = got.cam_depth[:, None], got.cam_seg[:, None]
    new[8], new[9], new[10] = got.bev_seg, got.bev_height, got.bev_mask
    return new
