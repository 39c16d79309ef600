"""Segmentation evaluation of the multi-task model: lidar-segmentation mIoU and Occ3D occupancy mIoU
(the reference's src/exps/nuscenes/base_exp.py:286-290 metric objects, :370-382 `training_step`,
:634-663 `validation_step`, :835-840 submission labels, :851-910 epoch ends).

The reference counts with torchmetrics' `JaccardIndex`, after a boolean index (`occ_logits[mask_camera]`:
a host synchronisation and a copy of half the logits) and an argmax.  Here the counting is the HIP
confusion-matrix pass of `evaluation.confusion_update` over the logits in place, and the per-reference-point
prediction is `evaluation.lidarseg_predict`; nothing leaves the device until `compute()`.
"""
import numpy as np
import torch
import torch.distributed as dist

from . import evaluation

# base_exp.py:222-224 (label_17_names): the 18 classes of the lidar-seg / Occ3D label space
CLASS_NAMES = ["other", "barrier", "bicycle", "bus", "car", "construction_vehicle", "motorcycle", "pedestrian",
               "traffic_cone", "trailer", "truck", "driveable_surface", "other_flat", "sidewalk", "terrain",
               "manmade", "vegetation", "free"]


class JaccardIndex:
    """Per-class intersection over union from an int64 confusion matrix (torchmetrics' multiclass
    `JaccardIndex(num_classes, ignore_index, average='none')`, the version the reference pins: 0.11.0).

    State: `confmat[target, pred]` and `invalid` (elements whose target -- or integer prediction -- lies
    outside [0, num_classes), which torchmetrics rejects).  This project's definition of the result:

        IoU_c = cm[c, c] / (sum_p cm[c, p] + sum_t cm[t, c] - cm[c, c]),   and 0.0 when that union is 0,

    as float64.  `compute()` raises ValueError while `invalid` is non-zero.  Elements whose target equals
    `ignore_index` are not counted; the entry AT `ignore_index` is unspecified (callers drop it)."""

    def __init__(self, num_classes, ignore_index=None, device="cuda"):
        self.num_classes, self.ignore_index = int(num_classes), ignore_index
        self.confmat = torch.zeros(self.num_classes, self.num_classes, dtype=torch.int64, device=device)
        self.invalid = torch.zeros((), dtype=torch.int64, device=device)

    def update(self, logits_or_preds, target, mask=None, class_window=None):
        """Logits [..., K] (prediction lo + argmax over `class_window` = (lo, hi), default all classes) or
        integer predictions shaped like `target`; `mask` (bool, like target) selects the elements counted."""
        evaluation.confusion_update(self.confmat, self.invalid, logits_or_preds, target, mask, class_window=class_window,
                             ignore_index=self.ignore_index)

    def reset(self):
        self.confmat.zero_()
        self.invalid.zero_()

    def sync(self, group=None):
        """Sum the state over the process group (what torchmetrics does at compute() under DDP); a no-op
        when torch.distributed is not initialised."""
        if dist.is_available() and dist.is_initialized():
            dist.all_reduce(self.confmat, op=dist.ReduceOp.SUM, group=group)
            dist.all_reduce(self.invalid, op=dist.ReduceOp.SUM, group=group)

    def compute(self):
        if int(self.invalid) != 0:
            raise ValueError(f"{int(self.invalid)} elements had a target (or prediction) outside "
                             f"[0, {self.num_classes})")
        cm = self.confmat.double()
        inter = cm.diagonal()
        union = cm.sum(1) + cm.sum(0) - inter
        return torch.where(union > 0, inter / union.clamp(min=1), torch.zeros_like(inter))


class SegEvaluator:
    """The reference's four metric objects (base_exp.py:286-290) and the code around them: lidar-seg IoU
    over num_seg_classes - 1 classes with class 0 ignored (predictions are 1 + argmax over classes 1:-1),
    occupancy IoU over num_seg_classes classes (the last one, "free", is left out of the mean)."""

    def __init__(self, num_seg_classes=len(CLASS_NAMES), class_names=None, device="cuda"):
        K = self.num_seg_classes = int(num_seg_classes)
        names = list(CLASS_NAMES if class_names is None else class_names)
        if len(names) != K:
            raise ValueError(f"{len(names)} class names for {K} classes")
        self.lidar_names, self.occ_names = names[1:-1], names          # unique_label_str, occ_label_str
        self.train_iou = JaccardIndex(K - 1, ignore_index=0, device=device)
        self.occ_train_iou = JaccardIndex(K, device=device)
        self.val_iou = JaccardIndex(K - 1, ignore_index=0, device=device)
        self.occ_val_iou = JaccardIndex(K, device=device)
        self.best_miou = self.best_occ_miou = 0.0

    @property
    def window(self):
        return (1, self.num_seg_classes - 1)

    def update_train(self, outputs, batch):
        """base_exp.py:370-382 on the 12 model outputs of a training forward and the 20-entry train batch."""
        pts_logits, occ_logits = outputs[8], outputs[10]
        inrange_labels, occ_semantics, mask_camera = batch[12], batch[16], batch[19]
        for logits, labels in zip(pts_logits, inrange_labels):
            self.train_iou.update(logits, labels, class_window=self.window)
        self.occ_train_iou.update(occ_logits, occ_semantics, mask_camera)

    def update_val(self, outputs, batch):
        """base_exp.py:645-660 on the (pts_logits, occ_logits, occ_density) of a lidar_seg=True forward and the
        15-entry validation batch."""
        pts_logits, occ_logits = outputs[0], outputs[1]
        ref_labels, ref_index, occ_semantics, mask_camera = batch[8], batch[9], batch[11], batch[14]
        for logits, idx, labels in zip(pts_logits, ref_index, ref_labels):
            dev = logits.device
            pred, bad = evaluation.lidarseg_predict(logits, idx.to(dev, non_blocking=True), len(labels), self.window)
            self.val_iou.update(pred, labels.to(dev, non_blocking=True))
            self.val_iou.invalid += bad                  # index_add_ rejects an index out of range
        self.occ_val_iou.update(occ_logits, occ_semantics, mask_camera)

    def validation_step(self, model, batch):
        """base_exp.py:634-663: the model in eval mode without gradients, lidar_seg=True, then update_val."""
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                outputs = model(batch[0], batch[1], inrange_pts=batch[6], lidar_seg=True)
            self.update_val(outputs, batch)
        finally:
            model.train(was_training)
        return outputs

    def epoch_end(self, prefix="val"):
        """base_exp.py:851-910: sync, {prefix}/mIoU = nanmean(iou[1:]), {prefix}/occ_mIoU = nanmean(occ_iou[:-1]),
        the per-class IoUs by name; best values are kept for prefix 'val'; the metrics are reset."""
        lidar, occ = (self.val_iou, self.occ_val_iou) if prefix == "val" else (self.train_iou, self.occ_train_iou)
        lidar.sync()
        occ.sync()
        iou = lidar.compute()[1:].cpu().numpy()
        occ_iou = occ.compute()[:-1].cpu().numpy()
        miou, occ_miou = float(np.nanmean(iou)), float(np.nanmean(occ_iou))
        if prefix == "val":
            self.best_miou = max(self.best_miou, miou)
            self.best_occ_miou = max(self.best_occ_miou, occ_miou)
        out = {f"{prefix}/mIoU": miou, f"{prefix}/occ_mIoU": occ_miou}
        out.update({f"{prefix}/iou/{n}": float(v) for n, v in zip(self.lidar_names, iou)})
        out.update({f"{prefix}/occ_iou/{n}": float(v) for n, v in zip(self.occ_names, occ_iou)})
        lidar.reset()
        occ.reset()
        return out

    def lidarseg_labels(self, pts_logits_batch, ref_index, ref_labels):
        """The submission labels of base_exp.py:835-840 (uint8, 1 .. K - 2 per reference point), one device
        tensor per sample; no files are written.  Raises ValueError on a reference index out of range."""
        out = []
        for logits, idx, labels in zip(pts_logits_batch, ref_index, ref_labels):
            pred, bad = evaluation.lidarseg_predict(logits, idx.to(logits.device), len(labels), self.window)
            if int(bad):
                raise ValueError(f"{int(bad)} points map outside the {len(labels)} reference points")
            out.append(pred.to(torch.uint8))
        return out


# =============================================================================================
# detection: nuScenes mAP, true-positive errors and NDS (det_evaluators.py:61-117)
# =============================================================================================
TP_ERRORS = ("trans_err", "scale_err", "orient_err", "vel_err", "attr_err")           # the records' error order
ERR_NAME_MAPPING = {"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE",
                    "attr_err": "mAAE"}                                                # det_evaluators.py:16-22


def _cummean(x):
    """Running mean that ignores NaN: 0 while no finite value has been seen, ones when there is none at all."""
    nan = np.isnan(x)
    if nan.all():
        return np.ones(len(x))
    count = np.cumsum(~nan)
    total = np.cumsum(np.where(nan, 0.0, x))
    return np.divide(total, count, out=np.zeros_like(total), where=count != 0)


def _score_keys(bits):
    """int64 keys that order like the fp32 scores whose bit patterns `bits` (int32) holds, by the rule of
    vamp_det_eval_update: -0 equals +0, a NaN of either sign and any payload lies above +inf and NaNs are equal.  (A
    float sort is not asked: the device's radix sort places a NaN by its bits, one with the sign bit set below -inf.)"""
    score = bits.view(torch.float32)
    u = (score + 0.0).view(torch.int32).long() & 0xffffffff
    keys = torch.where(u >= 0x80000000, 0xffffffff - u, u + 0x80000000)
    return torch.where(score != score, torch.full_like(keys, 0xffffffff), keys)


class DetEvaluator:
    """Streaming nuScenes detection scores (`detection_cvpr_2019` as DESIGN 8.19 restates it; parity with the
    devkit is unpinned): `update()` per validation batch runs `evaluation.det_eval_update` -- one HIP launch, no host
    synchronisation --, `compute()` at the epoch's end sorts the records per class on the device, brings them to
    the host and finishes the 101-point curves and the scores in float64; `reset()` starts over.

    class_names: the head's classes in label order; max_samples: the capacity in samples; max_dets: the width of
    the DetResult (tasks x post_max_size).  protocol: class_range ({name: metres}), dist_ths, dist_th_tp,
    max_boxes_per_sample, min_recall, min_precision, mean_ap_weight (the defaults are detection_cvpr_2019's)."""

    def __init__(self, class_names, max_samples, max_dets, device="cuda", *, min_recall=0.1, min_precision=0.1,
                 mean_ap_weight=5.0, **protocol):
        self.min_recall, self.min_precision, self.mean_ap_weight = float(min_recall), float(min_precision), float(mean_ap_weight)
        self.state = evaluation.DetEvalState.new(class_names, max_samples, max_dets, device, **protocol)
        self.class_names = self.state.class_names

    def update(self, det, gt_boxes, gt_labels, gt_attrs=None):
        evaluation.det_eval_update(self.state, det, gt_boxes, gt_labels, gt_attrs)

    def reset(self):
        self.state.reset()

    def test_step(self, model, batch):
        """base_exp.py:665-746 on the 15-entry validation batch: the model in eval mode without gradients, the
        boxes decoded on the device (get_bboxes_device), then update with the batch's ground truth (entries 4, 5).
        Returns the DetResult."""
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                outputs = model(batch[0], batch[1], inrange_pts=batch[6], lidar_seg=False)
                det = model.get_bboxes_device(outputs[0])
            self.update(det, batch[4], batch[5])
        finally:
            model.train(was_training)
        return det

    def _sorted_records(self):
        """The valid records ordered by class, then score descending, then slot descending (the devkit's reversed
        ascending sort of (score, index)), as host arrays, with the counters; the one synchronisation."""
        st = self.state
        words = st.state.cpu().numpy()                                   # the synchronisation
        errors = dict(zip(("samples with more than max_boxes_per_sample boxes",
                           f"(sample, class) pairs with more than {evaluation._capi.VAMP_DET_EVAL_GT_CAP} ground-truth boxes",
                           "labels outside the class list", "batches beyond max_samples"), words[1:5].tolist()))
        if any(errors.values()):
            raise ValueError("detection evaluation: " + ", ".join(f"{v} {k}" for k, v in errors.items() if v))
        nrec = int(words[0]) * st.max_dets
        rec = st.records[:nrec]
        word = rec[:, 1]
        idx = torch.nonzero((word >> 8) & 1).flatten().flip(0)           # slots, descending
        idx = idx[torch.sort(_score_keys(rec[idx, 0]), stable=True, descending=True).indices]
        idx = idx[torch.sort(word[idx] & 0xff, stable=True).indices]
        rec = rec[idx].cpu().numpy()
        npos = words[8:8 + len(self.class_names)]
        return rec, npos

    def compute(self, prefix="pts_bbox_NuScenes"):
        """{prefix}/{class}_AP_dist_{d}, {prefix}/{class}_{err}, {prefix}/mATE .. mAAE, {prefix}/NDS, {prefix}/mAP
        (det_evaluators.py:99-116, unrounded).  Raises ValueError while an error counter is non-zero."""
        st = self.state
        rec, npos = self._sorted_records()
        cls = rec[:, 1] & 0xff
        conf_all = rec[:, 0].copy().view(np.float32).astype(np.float64)
        tp_all = (rec[:, 1] >> 16) & 0xf
        err_all = rec[:, 2:7].copy().view(np.float32).astype(np.float64)
        tp_h = st.dist_ths.index(float(st.dist_th_tp))
        first = int(round(100 * self.min_recall)) + 1
        grid = np.linspace(0, 1, 101)
        out, aps, tps = {}, [], {e: [] for e in TP_ERRORS}
        for c, name in enumerate(self.class_names):
            sel = cls == c
            conf, bits, errs = conf_all[sel], tp_all[sel], err_all[sel]
            class_aps = []
            for h, dist in enumerate(st.dist_ths):
                tp = ((bits >> h) & 1).astype(bool)
                if npos[c] == 0 or not tp.any():                         # the "no predictions" curve
                    prec, conf_i, curves = np.zeros(101), np.zeros(101), {e: np.ones(101) for e in TP_ERRORS}
                else:
                    tpc, fpc = np.cumsum(tp).astype(np.float64), np.cumsum(~tp).astype(np.float64)
                    rec_c = tpc / float(npos[c])
                    prec = np.interp(grid, rec_c, tpc / (fpc + tpc), right=0)
                    conf_i = np.interp(grid, rec_c, conf, right=0)
                    curves = {}
                    if h == tp_h:
                        for k, e in enumerate(TP_ERRORS):
                            mean = _cummean(errs[tp, k])
                            curves[e] = np.interp(conf_i[::-1], conf[tp][::-1], mean[::-1])[::-1]
                ap = float(np.mean(np.clip(prec[first:] - self.min_precision, 0, None))) / (1.0 - self.min_precision)
                class_aps.append(ap)
                out[f"{prefix}/{name}_AP_dist_{dist}"] = ap
                if h == tp_h:
                    nz = np.nonzero(conf_i)[0]
                    last = int(nz[-1]) if len(nz) else 0
                    for e in TP_ERRORS:
                        if (name == "traffic_cone" and e in ("attr_err", "vel_err", "orient_err")) \
                                or (name == "barrier" and e in ("attr_err", "vel_err")):
                            v = float("nan")
                        else:
                            v = 1.0 if last < first else float(np.mean(curves[e][first:last + 1]))
                        out[f"{prefix}/{name}_{e}"] = v
                        tps[e].append(v)
            aps.append(float(np.mean(class_aps)))
        mean_ap = float(np.mean(aps))
        total = self.mean_ap_weight * mean_ap
        for e in TP_ERRORS:
            vals = np.asarray(tps[e])
            m = float(np.mean(vals[~np.isnan(vals)])) if (~np.isnan(vals)).any() else float("nan")
            out[f"{prefix}/{ERR_NAME_MAPPING[e]}"] = m
            total += max(1.0 - m, 0.0)
        out[f"{prefix}/NDS"] = total / (self.mean_ap_weight + len(TP_ERRORS))
        out[f"{prefix}/mAP"] = mean_ap
        return out
