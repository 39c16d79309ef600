"""Writes tests/golden/workspace_sizes.json: what every `*_bytes` entry point and both `*_workspace_layout` entry
points return for three descriptors each --

  smallest   the smallest one the family's validator accepts;
  odd        odd extents and region sizes that are no multiple of 256 bytes, so that every rounding and every padding of
             the layout shows in the number.  Where a layout holds the cell scan's regions the extents give 63 or 64
             scan tiles: `ntile` and `ntile + 4` ints round to 256 and 512 bytes there, so the four words behind
             `aux[ntile]` show (at 1 .. 60 tiles modulo 64 both round to the same size);
  bench      the shape of the step bench.py runs (CFG_B, one sample of six cameras) or, for the operators outside
             that step, the shapes the model has at that configuration.

    python tests/golden/make_workspace_sizes.py          # with the library of the commit whose layouts are to be kept

Host computations only: no GPU.  tests/test_workspace_sizes.py holds the library to the file; it is regenerated only
when a layout is changed on purpose."""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from vampire_amd import _capi as K                               # noqa: E402
from vampire_amd.config import CFG_B                             # noqa: E402
from vampire_amd.ops import lift_desc, render_desc               # noqa: E402

_spec = importlib.util.spec_from_file_location("test_workspace_sizes", os.path.join(os.path.dirname(HERE), "test_workspace_sizes.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


def S(name, **fields):
    return {"struct": name, "fields": fields}


def of(struct):
    return {"struct": type(struct).__name__, "fields": T.from_struct(struct)}


def pad8(v, fill=0):
    return list(v) + [fill] * (8 - len(v))


# ---- the hot path ----------------------------------------------------------------------------------------------------
LIFT = {
    "smallest": S("VampLiftDesc", B=1, N=1, C=4, D=1, fH=1, fW=1, Z=1, Y=1, X=1, use_depth=0, in_dtype=K.VAMP_F32),
    "odd": S("VampLiftDesc", B=3, N=5, C=12, D=7, fH=87, fW=97, Z=5, Y=37, X=43, use_depth=1, in_dtype=K.VAMP_BF16),
    "bench": of(lift_desc(CFG_B, 1, 6, CFG_B.mid_channels, K.VAMP_F32)),
}
_bounds = dict(lo=[-1.0, -1.0, -1.0], span=[2.0, 2.0, 2.0])
RENDER = {
    "smallest": S("VampRenderDesc", B=1, N=1, D=2, fH=1, fW=1, K=1, C=0, Z=2, Y=2, X=2, oZ=1, oY=1, oX=1,
                  density_mode=K.VAMP_DENSITY_SIGMOID, in_dtype=K.VAMP_F32, **_bounds),
    "odd": S("VampRenderDesc", B=3, N=5, D=7, fH=13, fW=29, K=17, C=13, Z=15, Y=37, X=69, oZ=3, oY=33, oX=41,
             density_mode=K.VAMP_DENSITY_SDF_LAPLACE, cat_seg=1, in_dtype=K.VAMP_BF16, **_bounds),
    "bench": of(render_desc(CFG_B, 1, 6, K.VAMP_F32)),
}
_A = RENDER["bench"]["fields"]
_vol = dict(Z=_A["Z"], Y=_A["Y"], X=_A["X"])
_occ = 200 * 200 * 16                                             # the occupancy grid's points
SAMPLE = {
    "smallest": [S("VampSampleDesc", B=1, C=1, Z=1, Y=1, X=1, in_dtype=K.VAMP_F32, **_bounds), 0],
    "odd": [S("VampSampleDesc", B=3, C=7, Z=15, Y=37, X=69, in_dtype=K.VAMP_BF16, **_bounds), 1001],
    "bench": [S("VampSampleDesc", B=1, C=_A["K"], in_dtype=K.VAMP_F32, **_vol, **_bounds), _occ],
}
_q = dict(density_mode=K.VAMP_DENSITY_SDF_LAPLACE, sem_dtype=K.VAMP_F32, den_dtype=K.VAMP_F32, **_bounds)
QUERY = {
    "smallest": S("VampQueryDesc", B=1, K=1, Z=1, Y=1, X=1, M=0, P_occ=0, **_q),
    "odd": S("VampQueryDesc", B=3, K=17, Z=15, Y=37, X=69, M=1001, want_sdf=1, P_occ=777, **_q),
    "bench": S("VampQueryDesc", B=1, K=_A["K"], M=30000, want_sdf=1, P_occ=_occ, occ_shared=1, **_vol, **_q),
}

# ---- the layers ------------------------------------------------------------------------------------------------------
CONV = {
    "smallest": S("VampConvDesc", B=1, cin=16, cout=16, Z=1, Y=1, X=8),
    "odd": S("VampConvDesc", B=3, cin=16, cout=32, Z=5, Y=37, X=44),
    "bench": S("VampConvDesc", B=1, cin=32, cout=32, Z=_A["Z"], Y=_A["Y"] // 2, X=_A["X"] // 2),
}
POOL = {
    "smallest": S("VampPoolDesc", B=1, C=1, P=1, nx=1, ny=1, nz=1, in_dtype=K.VAMP_F32),
    "odd": S("VampPoolDesc", B=3, C=13, P=1001, nx=229, ny=187, nz=5, in_dtype=K.VAMP_BF16),
    "bench": S("VampPoolDesc", B=1, C=80, P=6 * _A["D"] * _A["fH"] * _A["fW"], nx=128, ny=128, nz=1, in_dtype=K.VAMP_F32),
}
BN = {
    "smallest": S("VampBatchNormDesc", eps=1e-5, momentum=0.1, N=1, C=1, H=1, W=1, dtype=K.VAMP_F32, training=1, world=1),
    "odd": S("VampBatchNormDesc", eps=1e-5, momentum=0.1, N=3, C=13, H=37, W=43, dtype=K.VAMP_BF16, act=K.VAMP_BN_ACT_RELU,
             has_residual=1, training=1, world=3, update_running=1),
    "bench": S("VampBatchNormDesc", eps=1e-5, momentum=0.1, N=6, C=64, H=64, W=176, dtype=K.VAMP_BF16, act=K.VAMP_BN_ACT_RELU,
               training=1, world=1, update_running=1),
}

# ---- the losses, targets, labels, images, metrics and the update -------------------------------------------------------
CONF = {
    "smallest": S("VampConfDesc", B=1, S=0, K=1, layout=K.VAMP_SEG_ROWS, pred_dtype=K.VAMP_F32, target_dtype=K.VAMP_I64, Kc=1, lo=0, hi=1),
    "odd": S("VampConfDesc", B=3, S=1001, K=17, layout=K.VAMP_SEG_PLANES, pred_dtype=K.VAMP_BF16, target_dtype=K.VAMP_U8, Kc=19,
             lo=1, hi=17, ignore_index=255, use_ignore=1),
    "bench": S("VampConfDesc", B=1, S=_occ, K=_A["K"], layout=K.VAMP_SEG_PLANES, pred_dtype=K.VAMP_F32, target_dtype=K.VAMP_I64,
               Kc=_A["K"], lo=0, hi=_A["K"]),
}
_tasks = [1, 2, 2, 1, 2, 2]                                       # the CenterPoint head's classes per task
_det = dict(in_dtype=K.VAMP_F32, score_threshold=0.1, out_size_factor=4.0, voxel_size=[0.1, 0.1], pc_range=[-51.2, -51.2],
            post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0])
DET = {
    "smallest": S("VampDetDesc", B=1, T=1, H=1, W=1, ncls=pad8([1]), max_num=1, pre_max_size=1, post_max_size=1,
                  nms_kind=K.VAMP_NMS_CIRCLE, **_det),
    "odd": S("VampDetDesc", B=3, T=5, H=37, W=43, ncls=pad8([1, 2, 3, 4, 1]), max_num=501, pre_max_size=1000, post_max_size=83,
             nms_kind=K.VAMP_NMS_ROTATE, has_vel=1, **_det),
    "bench": S("VampDetDesc", B=1, T=6, H=128, W=128, ncls=pad8(_tasks), max_num=500, pre_max_size=1000, post_max_size=83,
               nms_kind=K.VAMP_NMS_CIRCLE, has_vel=1, use_score_threshold=1, use_center_range=1, **_det),
}
_tgt = dict(gaussian_overlap=0.1, out_size_factor=4, min_radius=2, label_dtype=K.VAMP_I64, voxel_size=[0.1, 0.1], pc_range=[-51.2, -51.2])
TGT = {
    "smallest": S("VampDetTargetDesc", B=1, T=1, M=0, ncls=pad8([1]), box_cols=7, code=8, max_objs=1, fh=1, fw=1, **_tgt),
    "odd": S("VampDetTargetDesc", B=3, T=5, M=33, ncls=pad8([1, 2, 3, 4, 1]), box_cols=9, code=10, max_objs=501, fh=37, fw=43, **_tgt),
    "bench": S("VampDetTargetDesc", B=1, T=6, M=30, ncls=pad8(_tasks), box_cols=9, code=10, max_objs=500, fh=128, fw=128, **_tgt),
}
DETLOSS = {
    "smallest": S("VampDetLossDesc", B=1, T=1, H=1, W=1, ncls=pad8([1]), code=8, max_objs=1, has_vel=0, code_weights=[1.0] * 10,
                  loss_bbox_weight=0.25),
    "odd": S("VampDetLossDesc", B=3, T=5, H=37, W=43, ncls=pad8([1, 2, 3, 4, 1]), code=10, max_objs=501, has_vel=1,
             code_weights=[1.0] * 10, loss_bbox_weight=0.25),
    "bench": S("VampDetLossDesc", B=1, T=6, H=128, W=128, ncls=pad8(_tasks), code=10, max_objs=500, has_vel=1,
               code_weights=[1.0] * 8 + [0.2, 0.2], loss_bbox_weight=0.25),
}
RGB = {
    "smallest": S("VampRgbLossDesc", N=1, C=1, H=176, W=176, data_range=1.0, k1=0.01, k2=0.03),
    "odd": S("VampRgbLossDesc", N=3, C=3, H=181, W=333, data_range=1.0, k1=0.01, k2=0.03),
    "bench": S("VampRgbLossDesc", N=6, C=3, H=256, W=704, data_range=1.0, k1=0.01, k2=0.03),
}
SEG = {
    "smallest": S("VampSegLossDesc", B=1, S=1, C=2, layout=K.VAMP_SEG_ROWS, label_dtype=K.VAMP_I64, w_ce=1.0, w_lv=1.0),
    "odd": S("VampSegLossDesc", B=3, S=1001, C=17, layout=K.VAMP_SEG_PLANES, label_dtype=K.VAMP_U8, w_ce=1.0, w_lv=1.0),
    "bench": S("VampSegLossDesc", B=1, S=_occ, C=_A["K"], layout=K.VAMP_SEG_PLANES, label_dtype=K.VAMP_I64, w_ce=1.0, w_lv=1.0),
}


def _terms(ns):
    t = [dict(n=n, kind=K.VAMP_REG_SMOOTH_L1 if i % 2 == 0 else K.VAMP_REG_MSE, side=K.VAMP_REG_SET, pred_dtype=K.VAMP_F32)
         for i, n in enumerate(ns)]
    return dict(T=len(ns), terms=t + [dict(n=0)] * (K.VAMP_REG_MAX_TERMS - len(ns)))


_rays = 6 * _A["fH"] * _A["fW"]
REG = {
    "smallest": S("VampRegLossDesc", **_terms([1])),
    "odd": S("VampRegLossDesc", **_terms([3000001, 4097, 77])),
    "bench": S("VampRegLossDesc", **_terms([_rays, 3 * _rays, _occ, 30000])),
}
_upd = dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01, max_norm=35.0, ema_decay=0.999, scale_mode=K.VAMP_UPDATE_SCALE_DYNAMIC)
UPDATE = {
    "smallest": S("VampParamUpdateDesc", n_param_chunks=0, n_buffer_chunks=1, **_upd),
    "odd": S("VampParamUpdateDesc", n_param_chunks=1001, n_buffer_chunks=7, **_upd),
    "bench": S("VampParamUpdateDesc", n_param_chunks=16384, n_buffer_chunks=128, **_upd),
}
_ll = dict(origin_x=-51.4, origin_y=-51.4, size=0.4, point_cols=4, z_lo=-5.0, z_hi=3.0)
LABELS = {
    "smallest": S("VampLidarLabelDesc", B=1, N=1, M=0, label_dtype=K.VAMP_U8, H=1, W=1, stride=1, raw_w=1, raw_h=1, ny=1, nx=1, **_ll),
    "odd": S("VampLidarLabelDesc", B=3, N=5, M=1001, label_dtype=K.VAMP_U8, H=52, W=116, stride=4, raw_w=1600, raw_h=900, ny=37,
             nx=43, **_ll),
    "bench": S("VampLidarLabelDesc", B=1, N=6, M=30000, label_dtype=K.VAMP_I64, H=256, W=704, stride=4, raw_w=1600, raw_h=900,
               ny=256, nx=256, **_ll),
}
_img = dict(out_dtype=K.VAMP_F32, to_rgb=1, mean=[123.675, 116.28, 103.53], std_inv=[1 / 58.395, 1 / 57.12, 1 / 57.375])
IMAGES = {
    "smallest": S("VampImageDesc", raw_b_stride=3, raw_n_stride=3, raw_row_stride=3, B=1, N=1, raw_h=1, raw_w=1, H=1, W=1, taps_x=1,
                  taps_y=1, foot_w=1, foot_h=1, **_img),
    "odd": S("VampImageDesc", raw_b_stride=5 * 37 * 131, raw_n_stride=37 * 131, raw_row_stride=131, B=3, N=5, raw_h=37, raw_w=43,
             H=13, W=29, taps_x=5, taps_y=7, foot_w=33, foot_h=17, **_img),
    "bench": S("VampImageDesc", raw_b_stride=6 * 900 * 4800, raw_n_stride=900 * 4800, raw_row_stride=4800, B=1, N=6, raw_h=900,
               raw_w=1600, H=256, W=704, taps_x=8, taps_y=8, foot_w=272, foot_h=48, **_img),
}
_ev = dict(dist_ths=[0.5, 1.0, 2.0, 4.0], dist_th_tp=2.0, score_dtype=K.VAMP_F32, gt_label_dtype=K.VAMP_I64)


def _classes(n):
    pad = K.VAMP_DET_EVAL_MAX_CLASSES - n
    return dict(num_classes=n, class_range=[50.0] * n + [0.0] * pad, attr_moving=[-1] * n + [0] * pad, attr_still=[-1] * n + [0] * pad)


EVAL = {
    "smallest": S("VampDetEvalDesc", B=1, M=1, G=0, box_cols=7, max_boxes_per_sample=1, max_samples=1, **_classes(1), **_ev),
    "odd": S("VampDetEvalDesc", B=3, M=83, G=33, box_cols=9, has_attrs=1, max_boxes_per_sample=77, max_samples=11, **_classes(7), **_ev),
    "bench": S("VampDetEvalDesc", B=1, M=500, G=30, box_cols=9, has_attrs=1, max_boxes_per_sample=500, max_samples=81, **_classes(10), **_ev),
}

# function -> {case -> argument list}
CASES = {
    "vamp_lift_workspace_bytes": {k: [d] for k, d in LIFT.items()},
    "vamp_lift_workspace_layout": {k: [d] for k, d in LIFT.items()},
    "vamp_render_workspace_bytes": {k: [d] for k, d in RENDER.items()},
    "vamp_render_samples_bytes": {k: [d] for k, d in RENDER.items()},
    "vamp_render_term_offset": {k: [d] for k, d in RENDER.items()},
    "vamp_render_bev_workspace_bytes": {k: [d] for k, d in RENDER.items()},
    "vamp_render_workspace_layout": {k: [d] for k, d in RENDER.items()},
    "vamp_sample_points_workspace_bytes": SAMPLE,
    "vamp_point_queries_workspace_bytes": {k: [d] for k, d in QUERY.items()},
    # (C, oZ, Cout): one workgroup tile | the 5 x 4 tile shape | the step's gate: mid_channels x oZ -> 80
    "vamp_gate_conv1x1_workspace_bytes": {"smallest": [1, 1, 1], "odd": [7, 9, 17], "bench": [_A["C"], _A["oZ"], 80]},
    "vamp_voxel_pooling_workspace_bytes": {k: [d] for k, d in POOL.items()},
    "vamp_upsample_trilinear_workspace_bytes": {"smallest": [1, 1, 1], "odd": [5, 37, 43], "bench": [_A["Z"] // 2, _A["Y"] // 2, _A["X"] // 2]},
    "vamp_resize2d_workspace_bytes": {"smallest": [1, 1, 1, 1], "odd": [13, 29, 52, 116], "bench": [_A["fH"], _A["fW"], 256, 704]},
    "vamp_conv3d_workspace_bytes": {k: [d] for k, d in CONV.items()},
    "vamp_conv3d_bf16_workspace_bytes": {k: [d] for k, d in CONV.items()},
    "vamp_conv3d_half_s2_workspace_bytes": {k: [d] for k, d in CONV.items()},
    "vamp_conv3d_epilogue_workspace_bytes": {"smallest": [CONV["smallest"], 1], "odd": [CONV["odd"], 2], "bench": [CONV["bench"], 1]},
    "vamp_confusion_workspace_bytes": {k: [d] for k, d in CONF.items()},
    # (P, num_ref)
    "vamp_lidarseg_workspace_bytes": {"smallest": [0, 0], "odd": [1001, 130001], "bench": [30000, 34720]},
    "vamp_det_workspace_bytes": {k: [d] for k, d in DET.items()},
    "vamp_det_targets_workspace_bytes": {k: [d] for k, d in TGT.items()},
    "vamp_det_loss_workspace_bytes": {k: [d] for k, d in DETLOSS.items()},
    "vamp_rgb_loss_workspace_bytes": {k: [d] for k, d in RGB.items()},
    "vamp_seg_loss_workspace_bytes": {k: [d] for k, d in SEG.items()},
    "vamp_seg_loss_kept_bytes": {k: [d] for k, d in SEG.items()},
    "vamp_reg_loss_workspace_bytes": {k: [d] for k, d in REG.items()},
    "vamp_param_update_workspace_bytes": {k: [d] for k, d in UPDATE.items()},
    "vamp_lidar_labels_workspace_bytes": {k: [d] for k, d in LABELS.items()},
    "vamp_camera_images_workspace_bytes": {k: [d] for k, d in IMAGES.items()},
    "vamp_det_eval_record_bytes": {k: [d] for k, d in EVAL.items()},
    "vamp_bn_workspace_bytes": {k: [d] for k, d in BN.items()},
}


def main():
    lib = K.load()
    assert sorted(CASES) == T.size_entry_points(), sorted(set(CASES) ^ set(T.size_entry_points()))
    out = []
    for fn, by_case in CASES.items():
        for case, args in by_case.items():
            want = T.call(lib, fn, args)
            ok = want["status"] == 0 if fn in T.LAYOUTS else (want > 0 or fn == "vamp_resize2d_workspace_bytes")
            assert ok, f"{fn} [{case}] refuses its descriptor: {lib.vamp_last_error()}"
            if fn in T.LAYOUTS and case == "odd":       # the scan's `ntile + 4` shows (see above)
                regions = K.LIFTWS_REGIONS if "lift" in fn else K.RENDERWS_REGIONS
                size = dict(zip(regions, want["layout"]["bytes"]))
                assert size["aux"] > size["bsum"] == size["boff"], (fn, size)
            out.append({"fn": fn, "case": case, "args": args, "want": want})
    with open(os.path.join(HERE, "workspace_sizes.json"), "w") as f:
        json.dump({"cases": out}, f, indent=1)
        f.write("\n")
    print(len(out), "cases of", len(CASES), "entry points")


if __name__ == "__main__":
    main()
