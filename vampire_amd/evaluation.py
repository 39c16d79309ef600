"""Evaluation and detection-head operators on plain tensors (Python over the C ABI): the segmentation metrics'
confusion-matrix pass and lidar-segmentation prediction, CenterPoint post-processing (decode + NMS), training
targets and the detection loss.  All work happens in hand-written HIP kernels reached through `_capi`; there is no CPU fallback."""
import dataclasses

import torch

from . import _capi
from ._tensors import (DTYPE_CODES, FLOAT_DTYPES, _accept, _dtype_code, _logit_layout, _stream, as_labels, as_mask,
                       check_out, list_dtype, need_device, pad_lists, refused, scratch, workspace_bytes)


# ===========================================================================
# segmentation metrics (base_exp.py:370-382, :634-663, :835-840)
# ===========================================================================
_TARGET_DTYPES = (torch.int64, torch.int32, torch.uint8)


def confusion_update(confmat, invalid, logits_or_preds, target, mask=None, *, class_window=None, ignore_index=None):
    """confmat[t, p] += 1 for every element with mask true and target t != ignore_index, where p =
    lo + argmax(logits[..., lo:hi]) (torch.argmax ties and NaNs) or the integer prediction itself; targets
    (and integer predictions) outside [0, Kc) add 1 to `invalid` instead.  confmat: int64 [Kc, Kc], invalid:
    int64 with one element, both device tensors, accumulated.  logits [..., K] fp32 | bf16 (fp16 promoted),
    target / mask shaped like logits[..., 0] (or like the integer predictions); target int64 | int32 | uint8.
    One HIP pass on the current stream; no host synchronisation, capturable in a graph."""
    x = logits_or_preds
    need_device("confusion_update", confmat, invalid, x, target, mask)
    if confmat.dtype != torch.int64 or confmat.dim() != 2 or confmat.shape[0] != confmat.shape[1] \
            or not confmat.is_contiguous():
        raise ValueError("confmat must be a contiguous int64 [Kc, Kc] tensor")
    if invalid.dtype != torch.int64 or invalid.numel() != 1:
        raise ValueError("invalid must be a one-element int64 tensor")
    Kc = confmat.shape[0]
    integer = not x.is_floating_point()
    if integer:
        if tuple(x.shape) != tuple(target.shape):
            raise ValueError(f"predictions {tuple(x.shape)} and target {tuple(target.shape)} differ in shape")
        layout, B, S, x, K = _capi.VAMP_SEG_ROWS, 1, x.numel(), as_labels(x, (torch.int64, torch.int32)), 1
        lo, hi = 0, 1
    else:
        x = _accept(x)
        if tuple(x.shape[:-1]) != tuple(target.shape):
            raise ValueError(f"logits {tuple(x.shape)} do not match target {tuple(target.shape)}")
        K = x.shape[-1]
        lo, hi = (0, K) if class_window is None else (int(class_window[0]), int(class_window[1]))
        layout, B, S, x = _logit_layout(x)
    target = as_labels(target, _TARGET_DTYPES)
    if mask is not None and tuple(mask.shape) != tuple(target.shape):
        raise ValueError(f"mask {tuple(mask.shape)} does not match target {tuple(target.shape)}")
    mask = as_mask(mask)
    d = _capi.VampConfDesc(B, S, K, layout, DTYPE_CODES[x.dtype], DTYPE_CODES[target.dtype], Kc, lo, hi,
                           0 if ignore_index is None else int(ignore_index), 0 if ignore_index is None else 1, 0)
    vamp = _capi.checked()
    nbytes = workspace_bytes(vamp.vamp_confusion_workspace_bytes, d,
                             lambda: vamp.vamp_confusion_update(d, None, None, None, None, None, None, 0, None))
    with torch.cuda.device(x.device):
        ws = scratch("confusion", x.device, nbytes)
        vamp.vamp_confusion_update(d, x, target, mask, confmat, invalid, ws, ws.numel(), _stream())
    return confmat


def lidarseg_predict(pts_logits, ref_index, num_ref, class_window):
    """The reference's lidar-segmentation prediction (base_exp.py:645-649, :835-838): zeros [num_ref, K],
    index_add_(0, ref_index, pts_logits), then lo + argmax over classes [lo, hi).  Sums run in increasing
    point order (bit-exact against a sequential CPU index_add_).  Returns (labels int64 [num_ref], invalid
    int64 0-dim: the number of points whose index lies outside [0, num_ref)).  HIP kernels on the current
    stream; no host synchronisation."""
    need_device("lidarseg_predict", pts_logits, ref_index)
    if pts_logits.dim() != 2 or ref_index.dim() != 1 or ref_index.shape[0] != pts_logits.shape[0]:
        raise ValueError(f"expected pts_logits [P, K] and ref_index [P], got {tuple(pts_logits.shape)} "
                         f"and {tuple(ref_index.shape)}")
    x = _accept(pts_logits).contiguous()
    idx = ref_index.long().contiguous()
    P, K = x.shape
    lo, hi = int(class_window[0]), int(class_window[1])
    num_ref = int(num_ref)
    labels = torch.empty(num_ref, dtype=torch.int64, device=x.device)
    invalid = torch.empty((), dtype=torch.int64, device=x.device)
    vamp = _capi.checked()
    with torch.cuda.device(x.device):
        ws = scratch("lidarseg", x.device, vamp.vamp_lidarseg_workspace_bytes(P, num_ref))
        vamp.vamp_lidarseg_predict(P, K, _dtype_code(x), lo, hi, x, idx, num_ref, labels, invalid, ws, ws.numel(),
                                  _stream())
    return labels, invalid


# ===========================================================================
# detection post-processing (bev_depth_head.py:381-494)
# ===========================================================================
_NMS_KINDS = {"circle": _capi.VAMP_NMS_CIRCLE, "size_aware_circle": _capi.VAMP_NMS_SIZE_AWARE,
              "rotate": _capi.VAMP_NMS_ROTATE}


@dataclasses.dataclass
class DetResult:
    """Fixed-capacity detections of a batch: boxes [B, T * P, 9 | 7] fp32, scores [B, T * P] (heatmap dtype),
    labels [B, T * P] int32, counts [B] int32; rows at or beyond counts[b] are zero."""
    boxes: torch.Tensor
    scores: torch.Tensor
    labels: torch.Tensor
    counts: torch.Tensor

    def to_list(self):
        """get_bboxes's return value, [[bboxes, scores, labels], ...] per sample (one host synchronisation)."""
        n = self.counts.tolist()
        return [[self.boxes[b, :k], self.scores[b, :k], self.labels[b, :k]] for b, k in enumerate(n)]


def _cfg(c, name, default=None):
    if isinstance(c, dict):
        return c.get(name, default)
    return getattr(c, name, default)


def _per_task(v, T, name):
    if v is None:
        return [0.0] * T
    if isinstance(v, (int, float)):
        return [float(v)] * T
    if len(v) < T:
        raise ValueError(f"test_cfg['{name}'] has {len(v)} entries for {T} tasks")
    return [float(x) for x in v[:T]]


def det_postprocess(task_preds, coder_cfg, test_cfg, num_classes, norm_bbox, out=None):
    """BEVDepthHead.get_bboxes on the device (vamp_det_postprocess): sigmoid, the deterministic top-K (score
    descending, flat index ascending), CenterPointBBoxCoder.decode, the score and centre filters and test_cfg's
    nms_type -- 'circle', 'size_aware_circle' or 'rotate' (rotated BEV IoU > nms_thr, after pre_max_size) --
    for every task and sample in four launches, without a host synchronisation (capturable in a graph).
    task_preds: the head's preds_dicts ([[{'heatmap', 'reg', 'height', 'dim', 'rot'[, 'vel']}], ...]);
    coder_cfg: the bbox_coder config (dict or CenterPointBBoxCoder); num_classes: classes per task.
    out: a DetResult of preallocated buffers to write (graph capture).  Returns a DetResult."""
    heads = [pd[0] for pd in task_preds]
    T = len(heads)
    if not 1 <= T <= 8 or len(num_classes) < T:
        raise ValueError(f"{T} tasks with {len(num_classes)} class counts (1 to 8 tasks)")
    keys = ["heatmap", "reg", "height", "dim", "rot"]
    has_vel = "vel" in heads[0]
    if has_vel:
        keys.append("vel")
    tensors = [[h[k] for k in keys] for h in heads]
    need_device("det_postprocess", tensors)
    dtype = heads[0]["heatmap"].dtype
    if dtype not in FLOAT_DTYPES or any(x.dtype != dtype for ts in tensors for x in ts):
        raise TypeError(f"head tensors must all be fp32, bf16 or fp16 of one dtype, got {dtype}")
    B, _, H, W = heads[0]["heatmap"].shape
    chans = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2}
    for t, h in enumerate(heads):
        if h["heatmap"].dim() != 4 or h["heatmap"].shape[0] != B or tuple(h["heatmap"].shape[2:]) != (H, W):
            raise ValueError(f"task {t}: heatmap {tuple(h['heatmap'].shape)} does not match [{B}, *, {H}, {W}]")
        if h["heatmap"].shape[1] != num_classes[t]:
            raise ValueError(f"task {t}: heatmap has {h['heatmap'].shape[1]} classes, num_classes says {num_classes[t]}")
        for k, c in chans.items():
            if k in keys and tuple(h[k].shape) != (B, c, H, W):
                raise ValueError(f"task {t}: {k} {tuple(h[k].shape)} is not [{B}, {c}, {H}, {W}]")
    tensors = [[x.contiguous() for x in ts] for ts in tensors]
    kind = test_cfg["nms_type"]
    if kind not in _NMS_KINDS:
        raise ValueError(f"nms_type {kind!r} is not one of {sorted(_NMS_KINDS)}")
    thr = _cfg(coder_cfg, "score_threshold")
    rng = _cfg(coder_cfg, "post_center_range")
    d = _capi.VampDetDesc()
    d.B, d.T, d.H, d.W = B, T, H, W
    for t in range(T):
        d.ncls[t] = num_classes[t]
    d.max_num = int(_cfg(coder_cfg, "max_num", 100))
    d.pre_max_size = int(test_cfg.get("pre_max_size", d.max_num))
    d.post_max_size = int(test_cfg["post_max_size"])
    d.nms_kind = _NMS_KINDS[kind]
    d.in_dtype = DTYPE_CODES[dtype]
    d.has_vel, d.norm_bbox = int(has_vel), int(bool(norm_bbox))
    d.use_score_threshold, d.use_center_range = int(thr is not None), int(rng is not None)
    # torch compares a tensor with a Python scalar in the tensor's dtype
    d.score_threshold = float(torch.tensor(float(thr), dtype=dtype)) if thr is not None else 0.0
    d.out_size_factor = float(_cfg(coder_cfg, "out_size_factor"))
    vs, pc = _cfg(coder_cfg, "voxel_size"), _cfg(coder_cfg, "pc_range")
    d.voxel_size[0], d.voxel_size[1] = float(vs[0]), float(vs[1])
    d.pc_range[0], d.pc_range[1] = float(pc[0]), float(pc[1])
    if rng is not None:
        for i in range(6):
            d.post_center_range[i] = float(rng[i])
    mr = _per_task(test_cfg.get("min_radius") if kind == "circle" else None, T, "min_radius")
    ts = _per_task(test_cfg.get("thresh_scale") if kind == "size_aware_circle" else None, T, "thresh_scale")
    nt = _per_task(test_cfg.get("nms_thr") if kind == "rotate" else None, T, "nms_thr")
    for t in range(T):
        d.min_radius[t], d.thresh_scale[t], d.nms_thr[t] = mr[t], ts[t], nt[t]
    vamp = _capi.checked()
    nbytes = workspace_bytes(vamp.vamp_det_workspace_bytes, d,
                             lambda: vamp.vamp_det_postprocess(d, None, None, None, None, None, None, 0, None))
    P, cs = d.post_max_size, 9 if has_vel else 7
    dev = heads[0]["heatmap"].device
    if out is None:
        out = DetResult(torch.empty(B, T * P, cs, dtype=torch.float32, device=dev),
                        torch.empty(B, T * P, dtype=dtype, device=dev),
                        torch.empty(B, T * P, dtype=torch.int32, device=dev),
                        torch.empty(B, dtype=torch.int32, device=dev))
    else:
        want = [(out.boxes, (B, T * P, cs), torch.float32), (out.scores, (B, T * P), dtype),
                (out.labels, (B, T * P), torch.int32), (out.counts, (B,), torch.int32)]
        for x, shape, dt in want:
            check_out(x, shape, dt, dev, "out buffer", terse=True)
    table = _det_task_table(T, [ts_ + [None] * (6 - len(keys)) for ts_ in tensors])
    with torch.cuda.device(dev):
        ws = scratch("det", dev, nbytes)
        vamp.vamp_det_postprocess(d, table, out.boxes, out.scores, out.labels, out.counts, ws, ws.numel(), _stream())
    return out


# ===========================================================================
# detection training targets (bev_depth_head.py:168-319)
# ===========================================================================
_LABEL_DTYPES = (torch.int32, torch.int64)


@dataclasses.dataclass
class DetTargets:
    """The training targets of a batch: `heat` holds the tasks' [B, ncls_t, fh, fw] heatmaps one after the other
    (fp32), anno [T, B, max_objs, code] fp32, inds [T, B, max_objs] int64, masks [T, B, max_objs] uint8."""
    heat: torch.Tensor
    anno: torch.Tensor
    inds: torch.Tensor
    masks: torch.Tensor
    ncls: tuple
    fh: int
    fw: int

    def heatmaps(self):
        B = self.anno.shape[1]
        return [h.view(B, n, self.fh, self.fw) for h, n in
                zip(self.heat.split([B * n * self.fh * self.fw for n in self.ncls]), self.ncls)]

    def as_tuple(self):
        """get_targets's return value: (heatmaps, anno_boxes, inds, masks), each a list over tasks of [B, ...]
        views of the buffers."""
        return self.heatmaps(), list(self.anno.unbind(0)), list(self.inds.unbind(0)), list(self.masks.unbind(0))


def _pack_targets_input(boxes, labels):
    """Per-sample lists ([n_b, 7 | 9] boxes, [n_b] labels) -> padded [B, M, 7 | 9], [B, M] (label -1) on the
    device, without a host synchronisation; tensors pass through."""
    if isinstance(boxes, torch.Tensor):
        if not isinstance(labels, torch.Tensor):
            raise ValueError("boxes is a packed tensor but labels is not")
        return boxes, labels
    if len(boxes) != len(labels) or len(boxes) == 0:
        raise ValueError(f"{len(boxes)} box tensors and {len(labels)} label tensors (one per sample, at least one)")
    list_dtype(boxes, "boxes", torch.float32, "fp32")
    list_dtype(labels, "labels")
    need_device("det_targets", list(boxes), list(labels))
    return pad_lists((boxes, labels), (0, -1))


def det_targets(boxes, labels, tasks_ncls, train_cfg, norm_bbox, out=None):
    """BEVDepthHead.get_targets on the device (vamp_det_targets): per task and sample the Gaussian heatmaps and
    the anno / ind / mask rows of the first max_objs boxes in the reference's slot order, with the reference's
    fp32 chain, in two launches and without a host synchronisation (capturable in a graph with packed inputs).
    boxes, labels: per-sample lists ([n_b, 7 | 9] fp32, [n_b] int32 | int64; packed on the device with label -1
    padding) or packed [B, M, 7 | 9] and [B, M] tensors whose padding rows carry label -1.  tasks_ncls: classes
    per task, labels flat over the tasks.  out: a DetTargets of preallocated buffers to write (graph capture).
    Returns a DetTargets; as_tuple() is get_targets's (heatmaps, anno_boxes, inds, masks)."""
    packed = isinstance(boxes, torch.Tensor)
    boxes, labels = _pack_targets_input(boxes, labels)
    if boxes.dtype != torch.float32:
        raise TypeError(f"boxes must be fp32, got {boxes.dtype}")
    if labels.dtype not in _LABEL_DTYPES:
        raise TypeError(f"labels must be int32 or int64, got {labels.dtype}")
    if packed:                             # (per-sample lists were checked before they were padded)
        need_device("det_targets", boxes, labels)
    if boxes.dim() != 3 or boxes.shape[2] not in (7, 9) or tuple(labels.shape) != tuple(boxes.shape[:2]):
        raise ValueError(f"expected boxes [B, M, 7 | 9] and labels [B, M], got {tuple(boxes.shape)} "
                         f"and {tuple(labels.shape)}")
    ncls = tuple(int(n) for n in tasks_ncls)
    T = len(ncls)
    if not 1 <= T <= 8:
        raise ValueError(f"{T} tasks (1 to 8)")
    B, Mb, cols = boxes.shape
    osf = train_cfg["out_size_factor"]
    fw, fh = int(train_cfg["grid_size"][0]) // osf, int(train_cfg["grid_size"][1]) // osf
    code = len(train_cfg["code_weights"])
    max_objs = int(train_cfg["max_objs"] * train_cfg["dense_reg"])
    d = _capi.VampDetTargetDesc()
    d.gaussian_overlap = float(train_cfg["gaussian_overlap"])
    d.B, d.T, d.M = B, T, Mb
    for t in range(T):
        d.ncls[t] = ncls[t]
    d.box_cols, d.code, d.max_objs, d.fh, d.fw = cols, code, max_objs, fh, fw
    d.out_size_factor, d.min_radius, d.norm_bbox = int(osf), int(train_cfg["min_radius"]), int(bool(norm_bbox))
    d.label_dtype = DTYPE_CODES[labels.dtype]
    vs, pc = train_cfg["voxel_size"], train_cfg["point_cloud_range"]
    d.voxel_size[0], d.voxel_size[1] = float(vs[0]), float(vs[1])
    d.pc_range[0], d.pc_range[1] = float(pc[0]), float(pc[1])
    vamp = _capi.checked()
    nbytes = workspace_bytes(vamp.vamp_det_targets_workspace_bytes, d,
                             lambda: vamp.vamp_det_targets(d, None, None, None, None, None, None, None, 0, None))
    dev = boxes.device
    boxes, labels = boxes.contiguous(), labels.contiguous()
    if out is None:
        out = DetTargets(torch.empty(B * sum(ncls) * fh * fw, dtype=torch.float32, device=dev),
                         torch.empty(T, B, max_objs, code, dtype=torch.float32, device=dev),
                         torch.empty(T, B, max_objs, dtype=torch.int64, device=dev),
                         torch.empty(T, B, max_objs, dtype=torch.uint8, device=dev), ncls, fh, fw)
    else:
        want = [(out.heat, (B * sum(ncls) * fh * fw,), torch.float32), (out.anno, (T, B, max_objs, code), torch.float32),
                (out.inds, (T, B, max_objs), torch.int64), (out.masks, (T, B, max_objs), torch.uint8)]
        for x, shape, dt in want:
            check_out(x, shape, dt, dev, "out buffer", terse=True)
        if tuple(out.ncls) != ncls or (out.fh, out.fw) != (fh, fw):
            raise ValueError(f"out was made for classes {out.ncls} on {out.fh} x {out.fw}, not {ncls} on {fh} x {fw}")
    with torch.cuda.device(dev):
        ws = scratch("det_targets", dev, nbytes)
        vamp.vamp_det_targets(d, boxes, labels, out.heat, out.anno, out.inds, out.masks, ws, ws.numel(), _stream())
    return out


# ===========================================================================
# detection loss (bev_depth_head.py:321-379)
# ===========================================================================
_LOSS_KEYS = ("heatmap", "reg", "height", "dim", "rot", "vel")
_LOSS_CHANS = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2}


def _pack_loss_targets(targets, dev):
    """A DetTargets passes through; get_targets's 4-tuple of per-task lists is stacked into one on the device
    (cat / stack: no host synchronisation)."""
    if isinstance(targets, DetTargets):
        return targets
    heat, anno, inds, masks = targets
    if not (len(heat) == len(anno) == len(inds) == len(masks)) or len(heat) == 0:
        raise ValueError("targets must be a DetTargets or (heatmaps, anno_boxes, inds, masks) lists of one length")
    need_device("det_loss", list(heat), list(anno), list(inds), list(masks))
    if any(h.dim() != 4 for h in heat):
        raise ValueError("every target heatmap must be [B, ncls, H, W]")
    return DetTargets(torch.cat([h.reshape(-1) for h in heat]), torch.stack(list(anno)), torch.stack(list(inds)),
                      torch.stack(list(masks)), tuple(h.shape[1] for h in heat), heat[0].shape[2], heat[0].shape[3])


def _det_task_table(T, rows):
    table = (_capi.VampDetTask * T)()
    for t, row in enumerate(rows):
        table[t] = _capi.VampDetTask(*[None if x is None else x.data_ptr() for x in row])
    return table


def _loss_table(tensors, nk, T):
    """The task table of a flat list of `nk` tensors per task: the predictions, or their gradients (None: not wanted)."""
    return _det_task_table(T, [list(tensors[t * nk:(t + 1) * nk]) + [None] * (6 - nk) for t in range(T)])


class _DetLoss(torch.autograd.Function):
    """loss, terms = apply(desc, nk, heat, anno, inds, masks, counts, *predictions): the predictions task by task
    in the order of _LOSS_KEYS (nk = 6 with vel, 5 without)."""

    @staticmethod
    def forward(ctx, desc, nk, heat, anno, inds, masks, counts, *preds):
        dev = heat.device
        T = desc.T
        loss = torch.empty((), dtype=torch.float32, device=dev)
        terms = torch.empty(T, 2, dtype=torch.float32, device=dev)
        vamp = _capi.checked()
        with torch.cuda.device(dev):
            ws = scratch("det_loss", dev, vamp.vamp_det_loss_workspace_bytes(desc))
            vamp.vamp_det_loss_forward(desc, _loss_table(preds, nk, T), heat, anno, inds, masks, counts, loss, terms, ws,
                                       ws.numel(), _stream())
        ctx.desc, ctx.nk = desc, nk
        ctx.save_for_backward(heat, anno, inds, masks, counts, *preds)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, grad_loss, _grad_terms):
        heat, anno, inds, masks, counts, *preds = ctx.saved_tensors
        desc, nk, T = ctx.desc, ctx.nk, ctx.desc.T
        dev = heat.device
        want = ctx.needs_input_grad[7:]
        grads = [torch.empty_like(x) if w else None for x, w in zip(preds, want)]
        if any(want):
            gl = grad_loss.to(torch.float32).contiguous()
            vamp = _capi.checked()
            with torch.cuda.device(dev):
                ws = scratch("det_loss", dev, vamp.vamp_det_loss_workspace_bytes(desc))
                vamp.vamp_det_loss_backward(desc, _loss_table(preds, nk, T), heat, anno, inds, masks, counts, gl,
                                            _loss_table(grads, nk, T), ws, ws.numel(), _stream())
        return (None,) * 7 + tuple(grads)


def det_loss_counts(desc, heat, masks):
    """counts [T, 2] fp32 = (number of heat == 1, sum of masks) per task (vamp_det_loss_counts, one launch)."""
    counts = torch.empty(desc.T, 2, dtype=torch.float32, device=heat.device)
    with torch.cuda.device(heat.device):
        _capi.checked().vamp_det_loss_counts(desc, heat, masks, counts, _stream())
    return counts


def det_loss(task_preds, targets, code_weights, loss_bbox_weight=0.25, *, counts=None):
    """BEVDepthHead.loss on the device (vamp_det_loss_*): the Gaussian focal loss of the clipped sigmoid heatmaps
    plus the code-weighted L1 loss of the box rows gathered at the targets' cells, summed over the tasks, in three
    launches (the counts and two for the loss; two more for the gradient, through autograd), without a host synchronisation, without float atomics
    and bitwise repeatable; capturable in a graph.  Returns the 0-dim fp32 loss; its attribute `terms` is the
    detached [T, 2] tensor of (heatmap, box) terms per task.
    task_preds: the head's preds_dicts ([[{'heatmap', 'reg', 'height', 'dim', 'rot'[, 'vel']}], ...]), fp32.
    Unlike the host loss, which replaces p['heatmap'] by its clipped sigmoid and adds p['anno_box'], this function
    leaves the dicts as they are.  targets: a DetTargets (det_targets) or get_targets's (heatmaps, anno_boxes,
    inds, masks) lists.  counts: None computes the averaging factors on the device and, when a process group is
    initialised, means the [T, 2] tensor over the ranks in one collective; a given [T, 2] fp32 device tensor of
    (positives, mask sum) per task is used as it is (the clamps to 1 and 1e-4 are applied by the kernels).
    Gradients go to the predictions that require them; a masked slot whose index lies outside the map is skipped
    (torch's gather would assert)."""
    heads = [pd[0] for pd in task_preds]
    T = len(heads)
    if not 1 <= T <= 8:
        raise ValueError(f"{T} tasks (1 to 8)")
    has_vel = "vel" in heads[0]
    keys = _LOSS_KEYS if has_vel else _LOSS_KEYS[:5]
    for t, h in enumerate(heads):
        if any(k not in h for k in keys) or ("vel" in h) != has_vel:
            raise ValueError(f"task {t}: heads {sorted(h)} do not match task 0's {list(keys)}")
    tensors = [[h[k] for k in keys] for h in heads]
    if any(x.dtype != torch.float32 for ts in tensors for x in ts):
        raise TypeError(f"head tensors must be fp32, got {sorted({str(x.dtype) for ts in tensors for x in ts})}")
    need_device("det_loss", tensors)
    dev = tensors[0][0].device
    tg = _pack_loss_targets(targets, dev)
    need_device("det_loss", tg.heat, tg.anno, tg.inds, tg.masks)
    if (tg.heat.dtype, tg.anno.dtype, tg.inds.dtype, tg.masks.dtype) != (torch.float32, torch.float32, torch.int64,
                                                                         torch.uint8):
        raise TypeError("targets must be fp32 heat and anno, int64 inds, uint8 masks")
    if heads[0]["heatmap"].dim() != 4:
        raise ValueError(f"heatmap {tuple(heads[0]['heatmap'].shape)} is not [B, ncls, H, W]")
    B, _, H, W = heads[0]["heatmap"].shape
    code = len(code_weights)
    if code != (10 if has_vel else 8):
        raise ValueError(f"{code} code weights for heads {'with' if has_vel else 'without'} vel (10 with, 8 without)")
    if len(tg.ncls) != T or (tg.fh, tg.fw) != (H, W):
        raise ValueError(f"targets of {len(tg.ncls)} tasks on {tg.fh} x {tg.fw}, predictions of {T} on {H} x {W}")
    if tg.anno.dim() != 4 or tuple(tg.anno.shape[:2]) != (T, B) or tg.anno.shape[3] != code:
        raise ValueError(f"anno {tuple(tg.anno.shape)} is not [{T}, {B}, max_objs, {code}]")
    K = tg.anno.shape[2]
    if tuple(tg.inds.shape) != (T, B, K) or tuple(tg.masks.shape) != (T, B, K):
        raise ValueError(f"inds {tuple(tg.inds.shape)} / masks {tuple(tg.masks.shape)} are not [{T}, {B}, {K}]")
    if tg.heat.numel() != B * sum(tg.ncls) * H * W:
        raise ValueError(f"heat holds {tg.heat.numel()} elements, not {B} x {sum(tg.ncls)} x {H} x {W}")
    for t, h in enumerate(heads):
        if tuple(h["heatmap"].shape) != (B, tg.ncls[t], H, W):
            raise ValueError(f"task {t}: heatmap {tuple(h['heatmap'].shape)} is not [{B}, {tg.ncls[t]}, {H}, {W}]")
        for k in keys[1:]:
            if tuple(h[k].shape) != (B, _LOSS_CHANS[k], H, W):
                raise ValueError(f"task {t}: {k} {tuple(h[k].shape)} is not [{B}, {_LOSS_CHANS[k]}, {H}, {W}]")
    d = _capi.VampDetLossDesc()
    d.B, d.T, d.H, d.W = B, T, H, W
    for t in range(T):
        d.ncls[t] = int(tg.ncls[t])
    d.code, d.max_objs, d.has_vel = code, K, int(has_vel)
    for c in range(code):
        d.code_weights[c] = float(code_weights[c])
    d.loss_bbox_weight = float(loss_bbox_weight)
    vamp = _capi.checked()
    if vamp.vamp_det_loss_workspace_bytes(d) == 0:
        raise refused(vamp, "det_loss", _capi.VampireHipError)
    heat, anno, inds, masks = tg.heat.contiguous(), tg.anno.contiguous(), tg.inds.contiguous(), tg.masks.contiguous()
    if counts is None:
        counts = det_loss_counts(d, heat, masks)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            from .multitask import reduce_mean
            counts = reduce_mean(counts)
    else:
        need_device("det_loss", counts)
        if counts.dtype != torch.float32:
            raise TypeError(f"counts must be fp32, got {counts.dtype}")
        if tuple(counts.shape) != (T, 2):
            raise ValueError(f"counts {tuple(counts.shape)} is not [{T}, 2]")
        counts = counts.detach().contiguous()
    flat = [x.contiguous() for ts in tensors for x in ts]
    loss, terms = _DetLoss.apply(d, len(keys), heat, anno, inds, masks, counts, *flat)
    loss.terms = terms
    return loss


# ===========================================================================
# detection scoring (det_evaluators.py:61-117, :254-274; base_exp.py:665-746)
# ===========================================================================
# the attribute names a ground-truth attribute index points into
ATTRIBUTE_NAMES = ("cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing",
                   "pedestrian.sitting_lying_down", "vehicle.moving", "vehicle.parked", "vehicle.stopped")
# detection_cvpr_2019's class ranges (metres)
CLASS_RANGE = {"car": 50.0, "truck": 50.0, "bus": 50.0, "trailer": 50.0, "construction_vehicle": 50.0,
               "pedestrian": 40.0, "motorcycle": 40.0, "bicycle": 40.0, "traffic_cone": 30.0, "barrier": 30.0}
# det_evaluators.py:24-35 and :254-274: class -> (attribute above 0.2 m/s, attribute at or below), '' for none
_DEFAULT_ATTRIBUTE = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
                      "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
                      "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "",
                      "traffic_cone": ""}


def predicted_attributes(name):
    """(moving, still): the attribute names det_evaluators.py:254-274 gives a prediction of class `name`."""
    default = _DEFAULT_ATTRIBUTE[name]
    if name in ("car", "construction_vehicle", "bus", "truck", "trailer"):
        moving = "vehicle.moving"
    elif name in ("bicycle", "motorcycle"):
        moving = "cycle.with_rider"
    else:
        moving = default
    still = "pedestrian.standing" if name == "pedestrian" else "vehicle.stopped" if name == "bus" else default
    return moving, still


@dataclasses.dataclass
class DetEvalState:
    """What det_eval_update accumulates, all on the device: `records` int32 [max_samples * max_dets, 8] (per
    detection row: the fp32 score's bits; class | valid << 8 | true-positive bits << 16; the bits of the five fp32
    errors trans, scale, orient, vel, attr; 0) and `state` int64 [24]: the sample cursor, the four error counters
    (samples over max_boxes_per_sample, (sample, class) pairs over the ground-truth cap, labels outside the class
    list, batches that did not fit) at 1 .. 4 and npos per class from 8 on."""
    records: torch.Tensor
    state: torch.Tensor
    class_names: tuple
    max_samples: int
    max_dets: int
    class_range: tuple
    dist_ths: tuple = (0.5, 1.0, 2.0, 4.0)
    dist_th_tp: float = 2.0
    max_boxes_per_sample: int = 500

    @classmethod
    def new(cls, class_names, max_samples, max_dets, device="cuda", class_range=None, **protocol):
        names = tuple(class_names)
        ranges = CLASS_RANGE if class_range is None else class_range
        missing = [n for n in names if n not in ranges or n not in _DEFAULT_ATTRIBUTE]
        if missing:
            raise ValueError(f"no class range or attribute rule for {missing}")
        if not 1 <= len(names) <= _capi.VAMP_DET_EVAL_MAX_CLASSES:
            raise ValueError(f"{len(names)} classes (1 to {_capi.VAMP_DET_EVAL_MAX_CLASSES})")
        self = cls(None, None, names, int(max_samples), int(max_dets), tuple(float(ranges[n]) for n in names), **protocol)
        self.dist_ths = tuple(float(t) for t in self.dist_ths)
        nbytes = _capi.checked().vamp_det_eval_record_bytes(self.desc(1, 0, 9, torch.float32, torch.int64, False))
        if nbytes == 0:
            raise refused(_capi.checked(), "det_eval")
        self.records = torch.zeros(nbytes // 32, 8, dtype=torch.int32, device=device)
        self.state = torch.zeros(_capi.VAMP_DET_EVAL_STATE_WORDS, dtype=torch.int64, device=device)
        return self

    def desc(self, B, G, cols, score_dtype, label_dtype, has_attrs):
        d = _capi.VampDetEvalDesc()
        d.B, d.M, d.G, d.box_cols = B, self.max_dets, G, cols
        d.score_dtype, d.gt_label_dtype, d.has_attrs = DTYPE_CODES[score_dtype], DTYPE_CODES[label_dtype], int(has_attrs)
        d.num_classes, d.max_boxes_per_sample, d.max_samples = len(self.class_names), int(self.max_boxes_per_sample), self.max_samples
        for h in range(4):
            d.dist_ths[h] = self.dist_ths[h]
        d.dist_th_tp = float(self.dist_th_tp)
        for c, name in enumerate(self.class_names):
            d.class_range[c] = self.class_range[c]
            flags = _capi.VAMP_DET_EVAL_HAS_ORIENT | _capi.VAMP_DET_EVAL_HAS_VEL | _capi.VAMP_DET_EVAL_HAS_ATTR
            if name == "traffic_cone":
                flags = 0
            elif name == "barrier":
                flags = _capi.VAMP_DET_EVAL_HAS_ORIENT | _capi.VAMP_DET_EVAL_HALF_PERIOD
            d.class_flags[c] = flags
            moving, still = predicted_attributes(name)
            d.attr_moving[c] = ATTRIBUTE_NAMES.index(moving) if moving else -1
            d.attr_still[c] = ATTRIBUTE_NAMES.index(still) if still else -1
        return d

    def reset(self):
        self.state.zero_()


def _pack_gt(gt_boxes, gt_labels, gt_attrs):
    """Per-sample lists -> padded [B, G, 7 | 9], [B, G] (label -1) and [B, G] int8 (attribute -1) on the device,
    without a host synchronisation; packed tensors pass through."""
    if isinstance(gt_boxes, torch.Tensor):
        if not isinstance(gt_labels, torch.Tensor) or not (gt_attrs is None or isinstance(gt_attrs, torch.Tensor)):
            raise ValueError("gt_boxes is a packed tensor but gt_labels or gt_attrs is not")
        return gt_boxes, gt_labels, gt_attrs
    lists = [gt_boxes, gt_labels] + ([] if gt_attrs is None else [gt_attrs])
    if any(len(l) != len(gt_boxes) for l in lists) or len(gt_boxes) == 0:
        raise ValueError(f"{[len(l) for l in lists]} tensors per list (one per sample, at least one)")
    need_device("det_eval_update", [list(l) for l in lists])
    list_dtype(gt_boxes, "gt_boxes", torch.float32, "fp32")
    list_dtype(gt_labels, "gt_labels")
    if gt_attrs is not None:
        list_dtype(gt_attrs, "gt_attrs", torch.int8, "int8")
    for s, (bx, lb) in enumerate(zip(gt_boxes, gt_labels)):
        if bx.dim() != 2 or lb.dim() != 1 or bx.shape[0] != lb.shape[0] \
                or (gt_attrs is not None and tuple(gt_attrs[s].shape) != tuple(lb.shape)):
            raise ValueError(f"sample {s}: expected gt boxes [n, 7 | 9] with labels (and attributes) [n], got "
                             f"{tuple(bx.shape)} and {tuple(lb.shape)}")
    if len({b.shape[1] for b in gt_boxes}) != 1:
        raise ValueError(f"gt_boxes differ in width: {sorted({b.shape[1] for b in gt_boxes})}")
    return pad_lists((gt_boxes, gt_labels, gt_attrs), (0, -1, -1))


def det_eval_update(state, det, gt_boxes, gt_labels, gt_attrs=None):
    """One validation batch of the nuScenes detection protocol (vamp_det_eval_update): per sample, class
    and distance threshold the greedy nearest-centre matching of the range-filtered detections, in score order, to
    the range-filtered ground truth, and the five true-positive errors of the matches at the 2 m threshold.  One
    launch on the current stream, then `cursor += B`; no host synchronisation, capturable in a graph (with packed
    ground truth).  state: a DetEvalState; det: a DetResult as det_postprocess returns it; gt_boxes, gt_labels: per-sample
    lists ([n_b, 9 | 7] fp32 in the ego frame, [n_b] int32 | int64) as the loader's get_gt gives them, or packed
    [B, G, 9 | 7] and [B, G] tensors whose padding rows carry label -1; gt_attrs: None (no ground truth has an
    attribute) or int8 indices into ATTRIBUTE_NAMES (-1: none), shaped like the labels.  Errors are counted in
    `state.state` (see DetEvalState); nothing is raised for them here."""
    if not isinstance(det, DetResult):
        raise TypeError(f"det must be a DetResult, got {type(det).__name__}")
    need_device("det_eval_update", det.boxes, det.scores, det.labels, det.counts)
    gtb, gtl, gta = _pack_gt(gt_boxes, gt_labels, gt_attrs)
    need_device("det_eval_update", gtb, gtl, gta)
    if det.boxes.dtype != torch.float32 or det.labels.dtype != torch.int32 or det.counts.dtype != torch.int32:
        raise TypeError("det must hold fp32 boxes, int32 labels and int32 counts")
    if det.scores.dtype not in FLOAT_DTYPES:
        raise TypeError(f"scores must be fp32, bf16 or fp16, got {det.scores.dtype}")
    if gtb.dtype != torch.float32:
        raise TypeError(f"gt_boxes must be fp32, got {gtb.dtype}")
    if gtl.dtype not in _LABEL_DTYPES:
        raise TypeError(f"gt_labels must be int32 or int64, got {gtl.dtype}")
    if gta is not None and gta.dtype != torch.int8:
        raise TypeError(f"gt_attrs must be int8, got {gta.dtype}")
    if det.boxes.dim() != 3 or det.boxes.shape[2] not in (7, 9):
        raise ValueError(f"det.boxes {tuple(det.boxes.shape)} is not [B, M, 7 | 9]")
    B, M, cols = det.boxes.shape
    if tuple(det.scores.shape) != (B, M) or tuple(det.labels.shape) != (B, M) or tuple(det.counts.shape) != (B,):
        raise ValueError(f"det holds scores {tuple(det.scores.shape)}, labels {tuple(det.labels.shape)}, counts "
                         f"{tuple(det.counts.shape)} for boxes {tuple(det.boxes.shape)}")
    if M != state.max_dets:
        raise ValueError(f"det is {M} rows wide, the state was made for {state.max_dets}")
    if gtb.dim() != 3 or gtb.shape[0] != B or gtb.shape[2] != cols or tuple(gtl.shape) != tuple(gtb.shape[:2]) \
            or (gta is not None and tuple(gta.shape) != tuple(gtl.shape)):
        raise ValueError(f"expected gt boxes [{B}, G, {cols}] with labels (and attributes) [{B}, G], got "
                         f"{tuple(gtb.shape)} and {tuple(gtl.shape)}")
    G = gtb.shape[1]
    d = state.desc(B, G, cols, det.scores.dtype, gtl.dtype, gta is not None)
    vamp = _capi.checked()
    if not vamp.vamp_det_eval_supported(d):
        raise refused(vamp, "det_eval_update")
    dev = det.boxes.device
    with torch.cuda.device(dev):
        vamp.vamp_det_eval_update(d, det.boxes.contiguous(), det.scores.contiguous(), det.labels.contiguous(),
                                  det.counts.contiguous(), gtb.contiguous(), gtl.contiguous(),
                                  None if gta is None else gta.contiguous(), state.records, state.state, _stream())
        state.state[:1] += B              # the cursor, on the same stream: a captured update appends on every replay
    return state
