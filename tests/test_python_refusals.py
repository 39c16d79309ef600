"""What the Python operators refuse, and with which words, is part of their interface: every deliberately wrong call of
CASES must raise the exception class and the message tests/golden/python_refusals.json records for it
(tests/golden/make_python_refusals.py wrote it from the commit the helpers of `_tensors` were factored out of).  Every
case raises in Python, or from a host-side refusal of the library, before any launch.  The cases that need no device
tensor -- host tensors everywhere, and every mistake an operator checks before it looks at devices -- run without a GPU.

`test_scratch_buffers`: which cached workspaces exist after each cached-scratch operator ran at two sizes on a stream
of its own -- one regrown buffer, or one per size -- under keys (kind, device, stream[, nbytes])."""
import json
import os
import re

import pytest
import torch

from vampire_amd import _tensors, ops
from vampire_amd import evaluation as E
from vampire_amd import images as I
from vampire_amd import labels as L
from vampire_amd import layers, losses, norm, optim

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_refusals.json")
f32, f64, i64, i32 = torch.float32, torch.float64, torch.int64, torch.int32
KEYS = ("heatmap", "reg", "height", "dim", "rot", "vel")
CHANS = {"reg": 2, "height": 1, "dim": 3, "rot": 2, "vel": 2}
NCLS = (1, 2)
CODER = dict(score_threshold=0.1, post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_num=10,
             out_size_factor=4, voxel_size=[0.1, 0.1], pc_range=[-1.6, -1.6])
TEST_CFG = dict(nms_type="circle", post_max_size=5, pre_max_size=10, min_radius=[1.0, 1.0])
TRAIN_CFG = dict(out_size_factor=4, grid_size=[32, 32, 1], code_weights=[1.0] * 10, max_objs=4, dense_reg=1,
                 gaussian_overlap=0.1, min_radius=2, voxel_size=[0.1, 0.1], point_cloud_range=[-1.6, -1.6, -5.0, 1.6, 1.6, 3.0])
AUGS = [[(0.5, (8, 8), (0, 0, 8, 8), False, 0.0)]]


def z(dev, *shape, dtype=f32):
    return torch.zeros(*shape, dtype=dtype, device=dev)


def heads(dev, ncls=NCLS, B=1, H=8, W=8):
    return [[{"heatmap": z(dev, B, n, H, W), **{k: z(dev, B, c, H, W) for k, c in CHANS.items()}}] for n in ncls]


# ---- the operators: valid tiny arguments on `dev`, and the call made from them ----------------------------------------
def confusion_args(dev):
    return dict(confmat=z(dev, 3, 3, dtype=i64), invalid=z(dev, 1, dtype=i64), x=z(dev, 16, 3), target=z(dev, 16, dtype=i64),
                mask=torch.ones(16, dtype=torch.bool, device=dev), class_window=None)


def confusion_call(a):
    E.confusion_update(a["confmat"], a["invalid"], a["x"], a["target"], a["mask"], class_window=a["class_window"])


def lidarseg_args(dev):
    return dict(pts_logits=z(dev, 16, 3), ref_index=z(dev, 16, dtype=i64), num_ref=4, class_window=(0, 3))


def det_post_args(dev):
    return dict(task_preds=heads(dev), coder_cfg=dict(CODER), test_cfg=dict(TEST_CFG), num_classes=list(NCLS),
                norm_bbox=True, out=None)


def det_result(dev, B=1, M=10, dtype=f32):
    return dict(boxes=z(dev, B, M, 9), scores=z(dev, B, M, dtype=dtype), labels=z(dev, B, M, dtype=i32),
                counts=z(dev, B, dtype=i32))


def det_post_call(a):
    out = a["out"] if a["out"] is None else E.DetResult(**a["out"])
    E.det_postprocess(a["task_preds"], a["coder_cfg"], a["test_cfg"], a["num_classes"], a["norm_bbox"], out)


def det_targets_args(dev):
    return dict(boxes=z(dev, 1, 4, 9), labels=torch.full((1, 4), -1, dtype=i64, device=dev), tasks_ncls=NCLS,
                train_cfg=dict(TRAIN_CFG), norm_bbox=True, out=None)


def det_targets_lists(dev):
    return dict(det_targets_args(dev), boxes=[z(dev, 4, 9)], labels=[z(dev, 4, dtype=i64)])


def targets(dev, T=2, B=1, K=4, code=10):
    return dict(heat=z(dev, B * sum(NCLS) * 64), anno=z(dev, T, B, K, code), inds=z(dev, T, B, K, dtype=i64),
                masks=z(dev, T, B, K, dtype=torch.uint8), ncls=NCLS, fh=8, fw=8)


def det_targets_call(a):
    out = a["out"] if a["out"] is None else E.DetTargets(**a["out"])
    E.det_targets(a["boxes"], a["labels"], a["tasks_ncls"], a["train_cfg"], a["norm_bbox"], out)


def det_loss_args(dev):
    return dict(task_preds=heads(dev), targets=targets(dev), code_weights=[1.0] * 10, counts=None)


def det_loss_call(a):
    tg = a["targets"]
    E.det_loss(a["task_preds"], E.DetTargets(**tg) if isinstance(tg, dict) else tg, a["code_weights"], counts=a["counts"])


def target_lists(dev):
    """get_targets's 4-tuple of per-task lists."""
    return [[z(dev, 1, n, 8, 8) for n in NCLS], [z(dev, 1, 4, 10) for _ in NCLS], [z(dev, 1, 4, dtype=i64) for _ in NCLS],
            [z(dev, 1, 4, dtype=torch.uint8) for _ in NCLS]]


def det_eval_args(dev):
    return dict(state=E.DetEvalState.new(("car", "pedestrian"), 2, 4, device=dev), det=det_result(dev, M=4),
                gt_boxes=[z(dev, 3, 9)], gt_labels=[z(dev, 3, dtype=i64)], gt_attrs=[z(dev, 3, dtype=torch.int8)])


def det_eval_packed(dev):
    return dict(det_eval_args(dev), gt_boxes=z(dev, 1, 3, 9), gt_labels=z(dev, 1, 3, dtype=i64),
                gt_attrs=z(dev, 1, 3, dtype=torch.int8))


def det_eval_call(a):
    E.det_eval_update(a["state"], E.DetResult(**a["det"]) if isinstance(a["det"], dict) else a["det"], a["gt_boxes"],
                      a["gt_labels"], a["gt_attrs"])


def rgb_args(dev):
    return dict(pred=z(dev, 1, 1, 176, 176), target=z(dev, 1, 1, 176, 176), data_range=1.0)


def seg_args(dev):
    return dict(logits=z(dev, 16, 3), labels=z(dev, 16, dtype=i64), mask=torch.ones(16, dtype=torch.bool, device=dev),
                ce_weight=1.0, lovasz_weight=1.0)


def reg_args(dev):
    return dict(pred=z(dev, 8), target=z(dev, 8), mask=torch.ones(8, dtype=torch.bool, device=dev), kind="smooth_l1", side="set")


def reg_call(a):
    losses.reg_losses([losses.RegTerm(**a)])


def labels_args(dev):
    return dict(points=z(dev, 1, 16, 4), labels=z(dev, 1, 16, dtype=torch.uint8), lidar2cam=torch.eye(4, device=dev).expand(1, 1, 4, 4),
                intrins=torch.eye(4, device=dev).expand(1, 1, 4, 4), aug=z(dev, 1, 1, 8, dtype=f64), final_dim=(8, 8),
                raw_dim=(16, 16), stride=1, bev=dict(x_bound=(-1.6, 1.6), y_bound=(-1.6, 1.6), z_bound=(-5.0, 3.0), size=0.4),
                counts=torch.full((1,), 16, dtype=i32, device=dev), out=None)


def labels_lists(dev):
    return dict(labels_args(dev), points=[z(dev, 16, 4)], labels=[z(dev, 16, dtype=torch.uint8)], counts=None)


def labels_out(dev):
    """Right buffers for labels_args, as a dict."""
    cam, bev = (1, 1, 8, 8), (1, 1, 1, 8, 8)
    return dict(cam_depth=z(dev, *cam), cam_seg=z(dev, *cam, dtype=i64), cam_fg=z(dev, *cam, dtype=torch.bool),
                bev_seg=z(dev, *bev, dtype=i64), bev_height=z(dev, *bev), bev_mask=z(dev, *bev, dtype=torch.bool))


def labels_call(a):
    a = dict(a)
    if isinstance(a["out"], dict):
        a["out"] = L.LidarLabels(**a["out"])
    L.lidar_labels(a.pop("points"), a.pop("labels"), **a)


def images_args(dev):
    return dict(raw=z(dev, 1, 1, 16, 16, 3, dtype=torch.uint8), plan=I.plan_camera_images(AUGS, (16, 16), (8, 8)).to(dev),
                mean=I.IMG_MEAN, dtype=f32, out=None, out_u8=None)


def images_call(a):
    a = dict(a)
    I.camera_images(a.pop("raw"), a.pop("plan"), **a)


def pooling_args(dev):
    return dict(geom_xyz=z(dev, 1, 1, 1, 2, 2, 3, dtype=i32), input_features=z(dev, 1, 1, 1, 2, 2, 4), voxel_num=(4, 4, 1))


def resize_args(dev):
    return dict(tensors=[z(dev, 1, 4, 4), z(dev, 2, 4, 4)], size=(8, 8))


def gate_args(dev):
    return dict(vo=z(dev, 1, 2, 2, 4, 4), vd=z(dev, 1, 1, 2, 4, 4), weight=z(dev, 3, 4))


def update_args(dev):
    return dict(model=torch.nn.Linear(2, 2).to(dev), lr=1e-3, betas=(0.9, 0.999))


def conv_args(dtype):
    return lambda dev: dict(x=z(dev, 1, 16, 2, 2, 8, dtype=dtype), weight=z(dev, 16, 16, 3, 3, 3, dtype=dtype))


def fused_args(dev):
    return dict(conv_args(f32)(dev), bias=z(dev, 16), residual=z(dev, 1, 16, 2, 2, 8), act="leaky_relu", stride=1)


def conv_heads_args(dev):
    """Segments as lists in HeadSegment's field order: channels, bias, act, out_dtype, negative_slope."""
    return dict(conv_args(f32)(dev), segments=[[8, z(dev, 8), "sigmoid", None, 0.01], [8, None, None, None, 0.01]])


def bn_tensors(dev, *names):
    C = 4
    x = lambda: z(dev, 2, C, 3, 3)
    vec = lambda: torch.ones(C, device=dev)
    every = dict(x=x, dy=x, y=x, residual=x, weight=vec, bias=vec, running_mean=vec, running_var=vec,
                 saved=lambda: z(dev, 3, C), rows=lambda: z(dev, 1, 2 * C + 1, dtype=f64),
                 num_batches_tracked=lambda: z(dev, 1, dtype=i64))
    return {n: every[n]() for n in names}


def bn_apply_args(dev):
    return dict(bn_tensors(dev, "x", "rows", "weight", "bias", "residual", "running_mean", "running_var", "num_batches_tracked"),
                act="relu", momentum=0.1)


def bn_backward_apply_args(dev):
    return dict(bn_tensors(dev, "dy", "x", "y", "saved", "weight"), rows=z(dev, 1, 8, dtype=f64), stat_rows=z(dev, 1, 9, dtype=f64),
                act="relu")


def bn_module_args(dev):
    return dict(bn_tensors(dev, "x", "residual"), dev=dev, channels=4, ctor={})


def bn_module_call(a):
    norm.BatchNormAct2d(a["channels"], act="relu", **a["ctor"]).to(a["dev"])(a["x"], a["residual"])


OPS = {
    "confusion_update": (confusion_args, confusion_call),
    "lidarseg_predict": (lidarseg_args, lambda a: E.lidarseg_predict(**a)),
    "det_postprocess": (det_post_args, det_post_call),
    "det_targets": (det_targets_args, det_targets_call),
    "det_targets[lists]": (det_targets_lists, det_targets_call),
    "det_loss": (det_loss_args, det_loss_call),
    "det_eval_new": (lambda dev: dict(class_names=("car",), max_samples=2, max_dets=4, device=dev),
                     lambda a: E.DetEvalState.new(**a)),
    "det_eval_update": (det_eval_args, det_eval_call),
    "det_eval_update[packed]": (det_eval_packed, det_eval_call),
    "rgb_loss": (rgb_args, lambda a: losses.rgb_loss(**a)),
    "seg_loss": (seg_args, lambda a: losses.seg_loss(**a)),
    "reg_losses": (reg_args, reg_call),
    "reg_loss": (reg_args, lambda a: losses.reg_loss(**a)),
    "lidar_labels": (labels_args, labels_call),
    "lidar_labels[lists]": (labels_lists, labels_call),
    "camera_images": (images_args, images_call),
    "voxel_pooling": (pooling_args, lambda a: layers.voxel_pooling(**a)),
    "resize_bilinear2d": (resize_args, lambda a: layers.resize_bilinear2d_pack(**a)),
    "gate_conv1x1": (gate_args, lambda a: ops._GateConvFn.apply(None, a["vo"], a["vd"], a["weight"], None)),
    "ParamUpdate": (update_args, lambda a: optim.ParamUpdate(**a)),
    "upsample_trilinear": (lambda dev: dict(x=z(dev, 1, 1, 2, 2, 2), size=(4, 4, 4)), lambda a: layers.upsample_trilinear(**a)),
    "conv3d_3x3x3": (conv_args(f32), lambda a: layers.conv3d_3x3x3(**a)),
    "conv3d_bf16": (conv_args(torch.bfloat16), lambda a: layers.conv3d_bf16(**a)),
    "conv3d_bf16_stride2": (conv_args(torch.bfloat16), lambda a: layers.conv3d_bf16_stride2(**a)),
    "conv3d_fused": (fused_args, lambda a: layers.conv3d_fused(**a)),
    "conv3d_heads": (conv_heads_args, lambda a: layers.conv3d_heads(**a)),
    "bn_partial_stats": (lambda dev: bn_tensors(dev, "x"), lambda a: norm.bn_partial_stats(**a)),
    "bn_apply": (bn_apply_args, lambda a: norm.bn_apply(**a)),
    "bn_apply_eval": (lambda dev: bn_tensors(dev, "x", "weight", "bias", "running_mean", "running_var"),
                      lambda a: norm.bn_apply_eval(**a)),
    "bn_backward_partial": (lambda dev: dict(bn_tensors(dev, "dy", "x", "y", "saved"), act="relu"),
                            lambda a: norm.bn_backward_partial(**a)),
    "bn_backward_apply": (bn_backward_apply_args, lambda a: norm.bn_backward_apply(**a)),
    "BatchNormAct2d": (bn_module_args, bn_module_call),
}


# ---- the mistakes: functions that spoil the arguments in place ---------------------------------------------------------
def at(a, path, fn):
    """a[path] = fn(a[path]); `path` a key or a tuple of keys / indices into nested dicts and lists."""
    path = path if isinstance(path, tuple) else (path,)
    for k in path[:-1]:
        a = a[k]
    a[path[-1]] = fn(a.get(path[-1]) if isinstance(a, dict) else a[path[-1]])


def host(*paths):
    """The tensors at `paths` moved to the host (no path: nothing, for the cases that run on host tensors alone)."""
    return lambda a: [at(a, p, lambda t: t.cpu()) for p in paths]


def put(path, value):
    return lambda a: at(a, path, lambda _: value(a) if callable(value) else value)


def cast(path, dtype):
    return lambda a: at(a, path, lambda t: t.to(dtype))


def like(path, *shape):
    """A zero tensor of another shape in the place of the one at `path` (same dtype and device)."""
    return lambda a: at(a, path, lambda t: t.new_zeros(shape))


def both(*mistakes):
    return lambda a: [m(a) for m in mistakes]


def misaligned(a):
    a["out"] = z(a["raw"].device, 3 * 8 * 8 + 1)[1:].view(1, 1, 3, 8, 8)


def nine_tasks(a):
    a["task_preds"], a["num_classes"] = heads(a["task_preds"][0][0]["heatmap"].device, (1,) * 9), [1] * 9


def huge_term(a):
    """2^31 elements: the one thing about a term that only the library refuses -- kinds, sides, dtypes and the term count
    are refused in Python first -- so the only way to the wrapper's `refused` line (reg_losses: the library's text).
    The term is one expanded bf16 element, which costs nothing until the wrapper makes it contiguous: 4 GiB and one
    torch copy, where every other case of this table uses a few kilobytes.  Nothing of the library's is launched."""
    a.update(pred=z(a["pred"].device, 1, dtype=torch.bfloat16).expand(1 << 31), target=0.0, mask=None)


H0 = ("task_preds", 0, 0)
HOST, GPU = False, True
# (operator, what is wrong, needs device tensors, the mistake)
CASES = [
    ("confusion_update", "host tensors", HOST, host()),
    *[("confusion_update", f"host {k}", GPU, host(k)) for k in ("confmat", "invalid", "x", "target", "mask")],
    ("confusion_update", "int32 confmat", GPU, cast("confmat", i32)),
    ("confusion_update", "float invalid", GPU, cast("invalid", f32)),
    ("confusion_update", "short target", GPU, like("target", 15)),
    ("confusion_update", "short mask", GPU, like("mask", 15)),
    ("confusion_update", "integer predictions of another shape", GPU, put("x", lambda a: z(a["x"].device, 15, dtype=i64))),
    ("confusion_update", "window the library refuses", GPU, put("class_window", (2, 1))),
    ("confusion_update", "host mask and int32 confmat", GPU, both(host("mask"), cast("confmat", i32))),
    ("lidarseg_predict", "host tensors", HOST, host()),
    *[("lidarseg_predict", f"host {k}", GPU, host(k)) for k in ("pts_logits", "ref_index")],
    ("lidarseg_predict", "short ref_index", GPU, like("ref_index", 15)),
    ("lidarseg_predict", "window the library refuses", GPU, put("class_window", (2, 2))),
    ("lidarseg_predict", "host ref_index, and short", GPU, both(like("ref_index", 15), host("ref_index"))),
    ("det_postprocess", "nine tasks", HOST, nine_tasks),
    ("det_postprocess", "host tensors", HOST, host()),
    *[("det_postprocess", f"host {k}", GPU, host(H0 + (k,))) for k in KEYS],
    ("det_postprocess", "host rot of task 1", GPU, host(("task_preds", 1, 0, "rot"))),
    ("det_postprocess", "float64 heatmap of task 1", GPU, cast(("task_preds", 1, 0, "heatmap"), f64)),
    ("det_postprocess", "reg with three channels", GPU, like(H0 + ("reg",), 1, 3, 8, 8)),
    ("det_postprocess", "heatmap against num_classes", GPU, put(("num_classes", 1), 3)),
    ("det_postprocess", "unknown nms_type", GPU, put(("test_cfg", "nms_type"), "soft")),
    ("det_postprocess", "post_max_size the library refuses", GPU, put(("test_cfg", "post_max_size"), 50)),
    ("det_postprocess", "out of another shape", GPU, put("out", lambda a: det_result(a["task_preds"][0][0]["reg"].device, M=9))),
    ("det_postprocess", "out with int64 labels", GPU,
     put("out", lambda a: dict(det_result(a["task_preds"][0][0]["reg"].device), labels=z(a["task_preds"][0][0]["reg"].device, 1, 10, dtype=i64)))),
    ("det_postprocess", "out with host counts", GPU,
     put("out", lambda a: dict(det_result(a["task_preds"][0][0]["reg"].device), counts=z("cpu", 1, dtype=i32)))),
    ("det_postprocess", "host reg and float64 heatmap", GPU, both(host(H0 + ("reg",)), cast(("task_preds", 1, 0, "heatmap"), f64))),
    ("det_targets", "host tensors", HOST, host()),
    ("det_targets", "float64 boxes", HOST, cast("boxes", f64)),
    ("det_targets", "int16 labels", HOST, cast("labels", torch.int16)),
    ("det_targets", "packed boxes, listed labels", HOST, put("labels", lambda a: [a["labels"][0]])),
    *[("det_targets", f"host {k}", GPU, host(k)) for k in ("boxes", "labels")],
    ("det_targets", "labels of another shape", GPU, like("labels", 1, 5)),
    ("det_targets", "nine tasks", GPU, put("tasks_ncls", (1,) * 9)),
    ("det_targets", "code the library refuses", GPU, put(("train_cfg", "code_weights"), [1.0] * 8)),
    ("det_targets", "out of another shape", GPU, put("out", lambda a: dict(targets(a["boxes"].device), heat=z(a["boxes"].device, 7)))),
    ("det_targets", "out with int32 inds", GPU,
     put("out", lambda a: dict(targets(a["boxes"].device), inds=z(a["boxes"].device, 2, 1, 4, dtype=i32)))),
    ("det_targets", "out made for other classes", GPU, put("out", lambda a: dict(targets(a["boxes"].device), ncls=(2, 1)))),
    ("det_targets", "host labels and int16 labels", GPU, both(cast("labels", torch.int16), host("labels"))),
    ("det_targets", "host boxes and labels of another shape", GPU, both(like("labels", 1, 5), host("boxes"))),
    ("det_targets[lists]", "host tensors", HOST, host()),
    ("det_targets[lists]", "float64 boxes", HOST, cast(("boxes", 0), f64)),
    ("det_targets[lists]", "two boxes, one label", HOST, put("boxes", lambda a: a["boxes"] * 2)),
    ("det_targets[lists]", "no sample", HOST, both(put("boxes", []), put("labels", []))),
    *[("det_targets[lists]", f"host {k}", GPU, host((k, 0))) for k in ("boxes", "labels")],
    ("det_targets[lists]", "labels of two dtypes", HOST, both(put("boxes", lambda a: a["boxes"] * 2),
                                                            put("labels", lambda a: [a["labels"][0], a["labels"][0].int()]))),
    ("det_targets[lists]", "host labels and float64 boxes", GPU, both(cast(("boxes", 0), f64), host(("labels", 0)))),
    ("det_targets[lists]", "int16 labels", GPU, cast(("labels", 0), torch.int16)),
    ("det_loss", "no task", HOST, put("task_preds", [])),
    ("det_loss", "a head without rot", HOST, lambda a: a["task_preds"][1][0].pop("rot")),
    ("det_loss", "float64 heads", HOST, cast(H0 + ("dim",), f64)),
    ("det_loss", "host tensors", HOST, host()),
    *[("det_loss", f"host {k}", GPU, host(H0 + (k,))) for k in KEYS],
    *[("det_loss", f"host targets.{k}", GPU, host(("targets", k))) for k in ("heat", "anno", "inds", "masks")],
    *[("det_loss", f"host element of the target lists' {n}", GPU, both(put("targets", lambda a: target_lists(a["targets"]["heat"].device)),
                                                                      host(("targets", i, 1))))
      for i, n in enumerate(("heatmaps", "anno_boxes", "inds", "masks"))],
    ("det_loss", "target lists of two lengths", GPU, both(put("targets", lambda a: target_lists(a["targets"]["heat"].device)),
                                                         lambda a: a["targets"][2].pop())),
    ("det_loss", "host counts", GPU, put("counts", z("cpu", 2, 2))),
    ("det_loss", "float64 counts", GPU, put("counts", lambda a: z(a["targets"]["heat"].device, 2, 2, dtype=f64))),
    ("det_loss", "counts of another shape", GPU, put("counts", lambda a: z(a["targets"]["heat"].device, 3, 2))),
    ("det_loss", "int32 inds", GPU, cast(("targets", "inds"), i32)),
    ("det_loss", "anno of another width", GPU, like(("targets", "anno"), 2, 1, 4, 8)),
    ("det_loss", "eight code weights", GPU, put("code_weights", [1.0] * 8)),
    ("det_loss", "heatmap of another size", GPU, like(H0 + ("heatmap",), 1, 1, 8, 4)),
    ("det_loss", "max_objs the library refuses", GPU, both(like(("targets", "anno"), 2, 1, 0, 10), like(("targets", "inds"), 2, 1, 0),
                                                          like(("targets", "masks"), 2, 1, 0))),
    ("det_loss", "host targets.heat and int32 inds", GPU, both(cast(("targets", "inds"), i32), host(("targets", "heat")))),
    ("det_loss", "host vel and host targets.anno", GPU, both(host(H0 + ("vel",)), host(("targets", "anno")))),
    ("det_loss", "host counts, and float64", GPU, put("counts", z("cpu", 2, 2, dtype=f64))),
    ("det_eval_new", "max_samples the library refuses", HOST, put("max_samples", 0)),
    ("det_eval_new", "a class without a range", HOST, put("class_names", ("car", "tram"))),
    ("det_eval_update", "det is a tuple", HOST, put("det", lambda a: tuple(a["det"].values()))),
    ("det_eval_update", "host tensors", HOST, host()),
    *[("det_eval_update", f"host det.{k}", GPU, host(("det", k))) for k in ("boxes", "scores", "labels", "counts")],
    *[("det_eval_update", f"host {k}", GPU, host((k, 0))) for k in ("gt_boxes", "gt_labels", "gt_attrs")],
    ("det_eval_update", "int64 det.labels", GPU, cast(("det", "labels"), i64)),
    ("det_eval_update", "float64 gt_boxes", GPU, cast(("gt_boxes", 0), f64)),
    ("det_eval_update", "int32 gt_attrs", GPU, cast(("gt_attrs", 0), i32)),
    ("det_eval_update", "scores of another shape", GPU, like(("det", "scores"), 1, 5)),
    ("det_eval_update", "det wider than the state", GPU, put("det", lambda a: det_result(a["gt_boxes"][0].device, M=5))),
    ("det_eval_update", "gt labels of another length", GPU, like(("gt_labels", 0), 2)),
    ("det_eval_update", "dist_ths the library refuses", GPU, lambda a: setattr(a["state"], "dist_ths", (0.0, 1.0, 2.0, 4.0))),
    ("det_eval_update", "host gt_boxes and float64 gt_boxes", GPU, both(cast(("gt_boxes", 0), f64), host(("gt_boxes", 0)))),
    ("det_eval_update", "host det.counts and int64 det.labels", GPU, both(cast(("det", "labels"), i64), host(("det", "counts")))),
    ("det_eval_update", "host det.boxes and host gt_labels", GPU, both(host(("det", "boxes")), host(("gt_labels", 0)))),
    ("det_eval_update[packed]", "packed boxes, listed labels", HOST, put("gt_labels", lambda a: [a["gt_labels"][0]])),
    *[("det_eval_update[packed]", f"host {k}", GPU, host(k)) for k in ("gt_boxes", "gt_labels", "gt_attrs")],
    ("det_eval_update[packed]", "int16 gt_labels", GPU, cast("gt_labels", torch.int16)),
    ("det_eval_update[packed]", "gt of another batch", GPU, like("gt_boxes", 2, 3, 9)),
    ("det_eval_update[packed]", "host gt_attrs and int16 gt_labels", GPU, both(cast("gt_labels", torch.int16), host("gt_attrs"))),
    ("rgb_loss", "float64 tensors", HOST, cast("pred", f64)),
    ("rgb_loss", "target of another shape", HOST, like("target", 1, 1, 176, 177)),
    ("rgb_loss", "five channels", HOST, both(like("pred", 1, 5, 176, 176), like("target", 1, 5, 176, 176))),
    ("rgb_loss", "data_range the library refuses", HOST, put("data_range", 0.0)),
    ("rgb_loss", "host tensors", HOST, host()),
    *[("rgb_loss", f"host {k}", GPU, host(k)) for k in ("pred", "target")],
    ("rgb_loss", "host target and a refused data_range", GPU, both(host("target"), put("data_range", 0.0))),
    ("seg_loss", "short labels", HOST, like("labels", 15)),
    ("seg_loss", "short mask", HOST, like("mask", 15)),
    ("seg_loss", "one class", HOST, like("logits", 16, 1)),
    ("seg_loss", "float labels", HOST, cast("labels", f32)),
    ("seg_loss", "host tensors", HOST, host()),
    *[("seg_loss", f"host {k}", GPU, host(k)) for k in ("logits", "labels", "mask")],
    ("seg_loss", "weight the library refuses", GPU, put("ce_weight", float("inf"))),
    ("seg_loss", "host mask and float labels", GPU, both(cast("labels", f32), host("mask"))),
    ("seg_loss", "host labels and a refused weight", GPU, both(host("labels"), put("ce_weight", float("inf")))),
    ("reg_losses", "unknown kind", HOST, put("kind", "l1")),
    ("reg_losses", "unknown side", HOST, put("side", "all")),
    ("reg_losses", "integer pred", HOST, cast("pred", i64)),
    ("reg_losses", "short target", HOST, like("target", 7)),
    ("reg_losses", "short mask", HOST, like("mask", 7)),
    ("reg_losses", "side clear without a mask", HOST, both(put("mask", None), put("side", "clear"))),
    ("reg_losses", "empty pred", HOST, both(like("pred", 0), like("target", 0), like("mask", 0))),
    ("reg_losses", "host tensors", HOST, host()),
    *[("reg_losses", f"host {k}", GPU, host(k)) for k in ("pred", "target", "mask")],
    ("reg_losses", "size the library refuses", GPU, huge_term),
    ("reg_losses", "host mask and empty tensors", GPU, both(like("pred", 0), like("target", 0), like("mask", 0), host("mask"))),
    ("reg_loss", "host tensors", HOST, host()),
    ("reg_loss", "host target", GPU, host("target")),
    ("lidar_labels", "host tensors", HOST, host()),
    ("lidar_labels", "packed points, listed labels", HOST, put("labels", lambda a: [a["labels"][0]])),
    *[("lidar_labels", f"host {k}", GPU, host(k)) for k in ("points", "labels", "counts", "lidar2cam", "intrins", "aug")],
    ("lidar_labels", "float64 points", GPU, cast("points", f64)),
    ("lidar_labels", "int32 labels", GPU, cast("labels", i32)),
    ("lidar_labels", "short labels", GPU, like("labels", 1, 15)),
    ("lidar_labels", "int64 counts", GPU, cast("counts", i64)),
    ("lidar_labels", "float32 aug", GPU, cast("aug", f32)),
    ("lidar_labels", "intrins of another shape", GPU, like("intrins", 1, 2, 4, 4)),
    ("lidar_labels", "stride that does not divide", GPU, put("stride", 3)),
    ("lidar_labels", "nothing to do", GPU, both(*[put(k, None) for k in ("lidar2cam", "intrins", "aug", "final_dim", "raw_dim", "bev")])),
    ("lidar_labels", "z_bound the library refuses", GPU, put(("bev", "z_bound"), (3.0, -5.0))),
    ("lidar_labels", "out without buffers", GPU, put("out", L.LidarLabels())),
    ("lidar_labels", "out of another dtype", GPU,
     put("out", lambda a: L.LidarLabels(cam_depth=z(a["points"].device, 1, 1, 8, 8, dtype=f64)))),
    ("lidar_labels", "host counts and int64 counts", GPU, both(cast("counts", i64), host("counts"))),
    ("lidar_labels", "host aug and float32 aug", GPU, both(cast("aug", f32), host("aug"))),
    ("lidar_labels", "host labels and float64 points", GPU, both(cast("points", f64), host("labels"))),
    ("lidar_labels[lists]", "host tensors", HOST, host()),
    ("lidar_labels[lists]", "counts beside lists", HOST, put("counts", lambda a: z("cpu", 1, dtype=i32))),
    ("lidar_labels[lists]", "two points, one label", HOST, put("points", lambda a: a["points"] * 2)),
    *[("lidar_labels[lists]", f"host {k}", GPU, host((k, 0))) for k in ("points", "labels")],
    ("lidar_labels[lists]", "float64 points", GPU, cast(("points", 0), f64)),
    ("lidar_labels[lists]", "short labels", GPU, like(("labels", 0), 15)),
    ("lidar_labels[lists]", "host labels and float64 points", GPU, both(cast(("points", 0), f64), host(("labels", 0)))),
    ("camera_images", "host tensors", HOST, host()),
    ("camera_images", "host raw", GPU, host("raw")),
    ("camera_images", "plan left on the host", GPU, put("plan", lambda a: I.plan_camera_images(AUGS, (16, 16), (8, 8)))),
    ("camera_images", "plan moved to the host", GPU, put("plan", lambda a: I.plan_camera_images(AUGS, (16, 16), (8, 8)).to("cpu"))),
    ("camera_images", "float raw", GPU, cast("raw", f32)),
    ("camera_images", "raw of another shape", GPU, like("raw", 1, 1, 16, 12, 3)),
    ("camera_images", "float16 output", GPU, put("dtype", torch.float16)),
    ("camera_images", "nothing to do", GPU, put("dtype", None)),
    ("camera_images", "two means", GPU, put("mean", (1.0, 2.0))),
    ("camera_images", "mean the library refuses", GPU, put("mean", (float("nan"), 0.0, 0.0))),
    ("camera_images", "out of another shape", GPU, put("out", lambda a: z(a["raw"].device, 1, 1, 3, 8, 9))),
    ("camera_images", "out off its 16-byte boundary", GPU, misaligned),
    ("camera_images", "int8 out_u8", GPU, put("out_u8", lambda a: z(a["raw"].device, 1, 1, 8, 8, 3, dtype=torch.int8))),
    ("camera_images", "host raw and float raw", GPU, both(cast("raw", f32), host("raw"))),
    ("voxel_pooling", "host tensors", HOST, host()),
    *[("voxel_pooling", f"host {k}", GPU, host(k)) for k in ("geom_xyz", "input_features")],
    ("resize_bilinear2d", "five tensors", HOST, put("tensors", lambda a: a["tensors"][:1] * 5)),
    ("resize_bilinear2d", "three sizes", HOST, put("size", (8, 8, 8))),
    ("resize_bilinear2d", "host tensors", HOST, host()),
    ("resize_bilinear2d", "host second tensor", GPU, host(("tensors", 1))),
    ("resize_bilinear2d", "float64 tensor", GPU, cast(("tensors", 0), f64)),
    ("resize_bilinear2d", "tensors of two sizes", GPU, like(("tensors", 1), 2, 4, 5)),
    ("resize_bilinear2d", "host second tensor and float64 first", GPU, both(cast(("tensors", 0), f64), host(("tensors", 1)))),
    ("gate_conv1x1", "host tensors", HOST, host()),
    *[("gate_conv1x1", f"host {k}", GPU, host(k)) for k in ("vo", "vd", "weight")],
    ("ParamUpdate", "host parameters", HOST, host()),
    ("ParamUpdate", "beta1 the library refuses", GPU, put("betas", (1.0, 0.999))),
    # ---- a host tensor as an out buffer, one at a time --------------------------------------------------------------
    *[("det_postprocess", f"out with host {k}", GPU, both(put("out", lambda a: det_result(a["task_preds"][0][0]["reg"].device)),
                                                         host(("out", k)))) for k in ("boxes", "scores", "labels")],
    *[("det_targets", f"out with host {k}", GPU, both(put("out", lambda a: targets(a["boxes"].device)), host(("out", k))))
      for k in ("heat", "anno", "inds", "masks")],
    *[("lidar_labels", f"out with host {k}", GPU, both(put("out", lambda a: labels_out(a["points"].device)), host(("out", k))))
      for k in ("cam_depth", "cam_seg", "cam_fg", "bev_seg", "bev_height", "bev_mask")],
    ("lidar_labels", "out without bev buffers", GPU, both(put("out", lambda a: labels_out(a["points"].device)),
                                                         put(("out", "bev_seg"), None))),
    ("camera_images", "host out", GPU, put("out", lambda a: z("cpu", 1, 1, 3, 8, 8))),
    ("camera_images", "host out_u8", GPU, put("out_u8", lambda a: z("cpu", 1, 1, 8, 8, 3, dtype=torch.uint8))),
    # ---- the layers: no dtype is refused by voxel_pooling and upsample_trilinear (they promote), and nothing about an
    # upsample's sizes by the library; the 16-bit kinds' library refusals are the fp32 kind's, asked once ---------------
    ("voxel_pooling", "geom_xyz of another size", GPU, like("geom_xyz", 1, 1, 1, 2, 3, 3)),
    ("voxel_pooling", "voxel_num the library refuses", GPU, put("voxel_num", (0, 4, 1))),
    ("upsample_trilinear", "host tensors", HOST, host()),
    ("upsample_trilinear", "four dimensions", GPU, like("x", 1, 2, 2, 2)),
    ("upsample_trilinear", "two sizes", GPU, put("size", (4, 4))),
    ("upsample_trilinear", "host x of four dimensions", GPU, both(like("x", 1, 2, 2, 2), host("x"))),
    ("conv3d_3x3x3", "host tensors", HOST, host()),
    *[("conv3d_3x3x3", f"host {k}", GPU, host(k)) for k in ("x", "weight")],
    ("conv3d_3x3x3", "bf16 operands", GPU, both(cast("x", torch.bfloat16), cast("weight", torch.bfloat16))),
    ("conv3d_3x3x3", "four dimensions", GPU, like("x", 16, 2, 2, 8)),
    ("conv3d_3x3x3", "weight for other channels", GPU, like("weight", 16, 32, 3, 3, 3)),
    ("conv3d_3x3x3", "channels the library refuses", GPU, both(like("x", 1, 8, 2, 2, 8), like("weight", 16, 8, 3, 3, 3))),
    ("conv3d_3x3x3", "host weight and bf16 x", GPU, both(cast("x", torch.bfloat16), host("weight"))),
    ("conv3d_bf16", "host tensors", HOST, host()),
    ("conv3d_bf16", "host x", GPU, host("x")),
    ("conv3d_bf16", "fp32 operands", GPU, both(cast("x", f32), cast("weight", f32))),
    ("conv3d_bf16", "operands of two dtypes", GPU, cast("weight", torch.float16)),
    ("conv3d_bf16", "weight for other channels", GPU, like("weight", 16, 32, 3, 3, 3)),
    ("conv3d_bf16_stride2", "host tensors", HOST, host()),
    ("conv3d_bf16_stride2", "host fp32 tensors", HOST, both(cast("x", f32), cast("weight", f32))),
    ("conv3d_bf16_stride2", "host weight", GPU, host("weight")),
    ("conv3d_bf16_stride2", "fp32 operands", GPU, both(cast("x", f32), cast("weight", f32))),
    ("conv3d_bf16_stride2", "host x and fp32 x", GPU, both(cast("x", f32), host("x"))),
    ("conv3d_bf16_stride2", "weight of four dimensions", GPU, like("weight", 16, 16, 3, 3)),
    ("conv3d_fused", "unknown activation", HOST, put("act", "relu")),
    ("conv3d_fused", "host tensors", HOST, host()),
    *[("conv3d_fused", f"host {k}", GPU, host(k)) for k in ("x", "weight", "bias", "residual")],
    ("conv3d_fused", "four dimensions", GPU, like("x", 16, 2, 2, 8)),
    ("conv3d_fused", "operands of two dtypes", GPU, cast("weight", torch.bfloat16)),
    ("conv3d_fused", "channels no kind takes", GPU, both(like("x", 1, 8, 2, 2, 8), like("weight", 16, 8, 3, 3, 3))),
    ("conv3d_fused", "stride 2 in fp32", GPU, put("stride", 2)),
    ("conv3d_fused", "short bias", GPU, like("bias", 15)),
    ("conv3d_fused", "residual of another shape", GPU, like("residual", 1, 16, 2, 2, 7)),
    ("conv3d_fused", "host bias, and short", GPU, both(like("bias", 15), host("bias"))),
    ("conv3d_heads", "five segments", HOST, put("segments", lambda a: a["segments"][1:] * 5)),
    ("conv3d_heads", "host tensors", HOST, host()),
    ("conv3d_heads", "host bias of a segment", GPU, host(("segments", 0, 1))),
    ("conv3d_heads", "unknown activation", GPU, put(("segments", 1, 2), "relu")),
    ("conv3d_heads", "float64 output", GPU, put(("segments", 1, 3), f64)),
    ("conv3d_heads", "more channels than the weight has", GPU, put(("segments", 1, 0), 16)),
    ("conv3d_heads", "short bias", GPU, like(("segments", 0, 1), 7)),
    # ---- batch norm: its operands raise "<name> must be a device tensor" ------------------------------------------------
    ("bn_partial_stats", "host tensors", HOST, host()),
    ("bn_partial_stats", "three dimensions", GPU, like("x", 2, 4, 9)),
    ("bn_partial_stats", "integer x", GPU, cast("x", i64)),
    ("bn_partial_stats", "empty batch the library refuses", GPU, like("x", 0, 4, 3, 3)),
    ("bn_partial_stats", "host integer x", GPU, both(cast("x", i64), host("x"))),
    ("bn_apply", "host tensors", HOST, host()),
    *[("bn_apply", f"host {k}", GPU, host(k)) for k in ("x", "rows", "weight", "bias", "residual", "running_mean", "running_var",
                                                        "num_batches_tracked")],
    ("bn_apply", "float32 rows", GPU, cast("rows", f32)),
    ("bn_apply", "rows of another width", GPU, like("rows", 1, 8)),
    ("bn_apply", "65 ranks", GPU, like("rows", 65, 9)),
    ("bn_apply", "residual of another shape", GPU, like("residual", 2, 4, 3, 2)),
    ("bn_apply", "running_mean alone", GPU, put("running_var", None)),
    ("bn_apply", "short running_var", GPU, like("running_var", 3)),
    ("bn_apply", "int32 num_batches_tracked", GPU, cast("num_batches_tracked", i32)),
    ("bn_apply", "float64 weight", GPU, cast("weight", f64)),
    ("bn_apply", "unknown activation", GPU, put("act", "gelu")),
    ("bn_apply", "momentum the library refuses", GPU, put("momentum", 2.0)),
    ("bn_apply", "host rows and float32 rows", GPU, both(cast("rows", f32), host("rows"))),
    ("bn_apply_eval", "host running_var", GPU, host("running_var")),
    ("bn_apply_eval", "float64 bias", GPU, cast("bias", f64)),
    *[("bn_backward_partial", f"host {k}", GPU, host(k)) for k in ("dy", "x", "y")],
    ("bn_backward_partial", "dy of another shape", GPU, like("dy", 2, 4, 3, 2)),
    ("bn_backward_partial", "saved of another shape", GPU, like("saved", 2, 4)),
    ("bn_backward_partial", "host saved", GPU, host("saved")),
    *[("bn_backward_apply", f"host {k}", GPU, host(k)) for k in ("weight", "rows", "stat_rows")],
    ("bn_backward_apply", "rows of another world", GPU, like("stat_rows", 2, 9)),
    ("bn_backward_apply", "rows of another width", GPU, like("rows", 1, 9)),
    ("BatchNormAct2d", "no momentum", HOST, put(("ctor", "momentum"), None)),
    ("BatchNormAct2d", "not affine", HOST, put(("ctor", "affine"), False)),
    ("BatchNormAct2d", "host tensors", HOST, host()),
    ("BatchNormAct2d", "host x", GPU, host("x")),
    ("BatchNormAct2d", "host residual", GPU, host("residual")),
    ("BatchNormAct2d", "three dimensions", GPU, like("x", 2, 4, 9)),
    ("BatchNormAct2d", "five channels", GPU, both(like("x", 2, 5, 3, 3), like("residual", 2, 5, 3, 3))),
    ("BatchNormAct2d", "residual of another dtype", GPU, cast("residual", torch.bfloat16)),
    ("BatchNormAct2d", "one value per channel", GPU, both(like("x", 1, 4, 1, 1), like("residual", 1, 4, 1, 1))),
    ("BatchNormAct2d", "host x of three dimensions", GPU, both(like("x", 2, 4, 9), host("x"))),
]
IDS = [f"{op}: {what}" for op, what, _, _ in CASES]


def outcome(op, gpu, mistake):
    """(exception class name, message) of one case, device names and addresses normalised; None if nothing is raised."""
    make, call = OPS[op]
    args = make("cuda" if gpu else "cpu")
    mistake(args)
    try:
        call(args)
    except Exception as e:           # noqa: BLE001 -- the class is what is compared
        text = re.sub(r"0x[0-9a-fA-F]+", "0xADDR", re.sub(r"cuda:\d+", "cuda:N", str(e)))
        return [type(e).__name__, text], e
    return None, None


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_covers_every_case_and_every_site(recorded):
    assert len(set(IDS)) == len(IDS)
    assert sorted(recorded["cases"]) == sorted(IDS)
    hit = {tuple(s) for c in recorded["cases"].values() for s in c["sites"]}
    assert recorded["sites"] and all(tuple(s) in hit for s in recorded["sites"])


def _replay(recorded, op, what, gpu, mistake):
    got, _ = outcome(op, gpu, mistake)
    assert got == recorded["cases"][f"{op}: {what}"]["raises"]


@pytest.mark.parametrize("op,what,gpu,mistake", [c for c in CASES if not c[2]], ids=[i for i, c in zip(IDS, CASES) if not c[2]])
def test_refusal_without_gpu(recorded, op, what, gpu, mistake):
    _replay(recorded, op, what, gpu, mistake)


@pytest.mark.gpu
@pytest.mark.parametrize("op,what,gpu,mistake", [c for c in CASES if c[2]], ids=[i for i, c in zip(IDS, CASES) if c[2]])
def test_refusal_on_device(recorded, op, what, gpu, mistake):
    _replay(recorded, op, what, gpu, mistake)


# ---- the cached workspaces ---------------------------------------------------------------------------------------------
def _grad(t):
    return t.requires_grad_(True)


def _confusion(dev, n):
    a = confusion_args(dev)
    E.confusion_update(a["confmat"], a["invalid"], z(dev, 1 << (10 + 8 * n), 3), z(dev, 1 << (10 + 8 * n), dtype=i64))


def _det_heads(dev, n):
    return heads(dev, B=1 + 15 * n, H=8 + 8 * n, W=8 + 8 * n)


def _det_targets(dev, n):
    cfg = dict(TRAIN_CFG, grid_size=[32 + 32 * n] * 2 + [1], max_objs=4 + 60 * n)
    return E.det_targets(z(dev, 1 + 15 * n, 4, 9), torch.full((1 + 15 * n, 4), -1, dtype=i64, device=dev), NCLS, cfg, True)


def _det_loss(dev, n):
    preds = _det_heads(dev, n)
    for k in KEYS:
        _grad(preds[0][0][k])
    E.det_loss(preds, _det_targets(dev, n), [1.0] * 10).backward()


def _labels(dev, n):
    a = dict(labels_args(dev), final_dim=(8 + 56 * n, 8 + 56 * n), counts=None)
    a["bev"] = dict(a["bev"], size=0.4 / (1 + 7 * n))
    labels_call(a)


def _images(dev, n):
    side = 8 + 56 * n
    augs = [[(0.5, (side, side), (0, 0, side, side), False, 0.0)]] * (1 + n)
    I.camera_images(z(dev, 1 + n, 1, 2 * side, 2 * side, 3, dtype=torch.uint8), I.plan_camera_images(augs, (2 * side,) * 2, (side,) * 2).to(dev))


def _batch_norm(dev, n):
    bn = norm.BatchNormAct2d(4 + 60 * n, act="relu").to(dev)
    bn(_grad(z(dev, 2, 4 + 60 * n, 3, 3 + 2 * norm.BN_CHUNK * n))).sum().backward()


def _conv(kind, dtype):
    def run(dev, n):
        x, w = _grad(z(dev, 1 + n, 16, 2, 2 + 2 * n, 8, dtype=dtype)), _grad(z(dev, 16 + 16 * n, 16, 3, 3, 3, dtype=dtype))
        layers._Conv3dFn.apply(kind, x, w).sum().backward()
    return run


def _conv_epilogue(dev, n):
    x, w, b = _grad(z(dev, 1 + n, 16, 2, 2 + 2 * n, 8)), _grad(z(dev, 16 + 16 * n, 16, 3, 3, 3)), _grad(z(dev, 16 + 16 * n))
    layers.conv3d_fused(x, w, bias=b, act="leaky_relu").sum().backward()


def _lidarseg(dev, n):
    P = 16 << (8 * n)
    E.lidarseg_predict(z(dev, P, 3), z(dev, P, dtype=i64), P // 4, (0, 3))


def _pooling(dev, n):
    layers.voxel_pooling(z(dev, 1, 1, 1, 2, 2, 3, dtype=i32), z(dev, 1, 1, 1, 2, 2, 4), (4 << (5 * n), 4 << (5 * n), 1))


def _resize2d(dev, n):
    layers.resize_bilinear2d(_grad(z(dev, 1, 4 + 60 * n, 4 + 60 * n)), (8 + 120 * n,) * 2).sum().backward()


def _upsample(dev, n):
    layers.upsample_trilinear(_grad(z(dev, 1, 1, 2, 2 + 6 * n, 2)), (4, 4 + 12 * n, 4)).sum().backward()


# operator -> (the kind its buffers are kept under, one buffer per size?, the call at size n = 0 | 1)
CACHED = {
    "confusion_update": ("confusion", False, _confusion),
    "lidarseg_predict": ("lidarseg", False, _lidarseg),
    "det_postprocess": ("det", False, lambda dev, n: E.det_postprocess(_det_heads(dev, n), CODER, TEST_CFG, NCLS, True)),
    "det_targets": ("det_targets", False, _det_targets),
    "det_loss": ("det_loss", False, _det_loss),
    "lidar_labels": ("lidar_labels", False, _labels),
    "camera_images": ("camera_images", False, _images),
    "batch_norm": ("batch_norm", False, _batch_norm),
    "voxel_pooling": ("voxel_pooling", False, _pooling),
    "resize_bilinear2d": ("resize2d", False, _resize2d),
    "upsample_trilinear": ("upsample_trilinear", True, _upsample),
    "conv3d_3x3x3": ("conv", True, _conv("fp32", f32)),
    "conv3d_bf16": ("conv16", True, _conv("half", torch.bfloat16)),
    "conv3d_bf16_stride2": ("conv16s2", True, _conv("half_s2", torch.bfloat16)),
    "conv3d_fused": ("convepi", True, _conv_epilogue),
}


@pytest.mark.gpu
def test_scratch_buffers(monkeypatch):
    """Every cached-scratch operator at a small shape, then at a larger one, on a stream no other test has used.  The
    regrowing operators then hold ONE buffer, of at least the larger size; the per-size operators one per size (DESIGN
    8.26; which operator does which is the parent commit's behaviour, listed in CACHED).  resize2d's workspace is
    empty at every size, so it asks for no buffer at all."""
    asked = {}

    def spy(kind, device, nbytes, **kw):
        asked.setdefault(kind, []).append(nbytes)
        return _tensors.scratch(kind, device, nbytes, **kw)

    for mod in (E, L, I, norm, layers):
        monkeypatch.setattr(mod, "scratch", spy)
    dev = torch.device("cuda", torch.cuda.current_device())
    used = {k[2] for k in _tensors._scratch}       # (torch hands out pooled streams: one an earlier test had comes back)
    stream = next(s for s in (torch.cuda.Stream(dev, priority=-(i % 2)) for i in range(128)) if s.cuda_stream not in used)
    with torch.cuda.stream(stream):
        for name, (kind, per_size, call) in CACHED.items():
            call(dev, 0)
            first = list(asked.get(kind, []))
            call(dev, 1)
            later = asked.get(kind, [])[len(first):]
            print(name, kind, first, later)
            if kind != "resize2d":                 # the larger shape does need more, and more than the floor of 256 bytes
                assert first and later and max(later) > max(max(first), 256), (name, first, later)
    stream.synchronize()
    mine = [k for k in _tensors._scratch if len(k) >= 3 and k[2] == stream.cuda_stream]
    for k in mine:
        assert isinstance(k[0], str) and k[1] == dev and len(k) in (3, 4), k
        assert len(k) == 3 or _tensors._scratch[k].numel() == max(k[3], 256), k
    assert "resize2d" not in asked and {k[0] for k in mine} == set(asked)
    for name, (kind, per_size, _) in CACHED.items():
        keys = [k for k in mine if k[0] == kind]
        if kind == "resize2d":
            assert keys == [], name
        elif per_size:
            assert sorted(keys) == sorted((kind, dev, stream.cuda_stream, n) for n in set(asked[kind])) and len(keys) == 2, (name, keys)
        else:
            assert keys == [(kind, dev, stream.cuda_stream)], (name, keys)
            assert _tensors._scratch[keys[0]].numel() >= max(asked[kind]), (name, asked[kind])
