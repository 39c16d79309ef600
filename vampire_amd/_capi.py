"""ctypes binding of include/vampire_hip.h (the C-ABI HIP library).

There is deliberately no fallback: if the shared library is missing or a symbol
does not resolve, importing the ops raises.  The product path never routes
through oracle/ or any CPU implementation.
"""
import ctypes as C
import os
import types
import typing

# torch must bring in ITS libamdhip64 first: a second HIP runtime (the system copy this
# library would otherwise pull in) sees no device inside a torch process.
import torch

from .build import lib_path

ABI_VERSION = 16

VAMP_F32, VAMP_BF16, VAMP_F16 = 0, 1, 2
VAMP_DENSITY_SIGMOID, VAMP_DENSITY_SDF_LAPLACE = 0, 1
VAMP_I64, VAMP_I32, VAMP_U8 = 3, 4, 5
VAMP_SEG_ROWS, VAMP_SEG_PLANES = 0, 1
VAMP_REG_MAX_TERMS, VAMP_REG_TILE = 8, 4096
VAMP_REG_SMOOTH_L1, VAMP_REG_MSE = 0, 1
VAMP_REG_SET, VAMP_REG_CLEAR, VAMP_REG_BOTH = 0, 1, 2
VAMP_RESIZE2D_MAX_SEGS, VAMP_RESIZE2D_PLANE_GROUP, VAMP_RESIZE2D_BAND_ROWS, VAMP_RESIZE2D_COL_CHUNK = 4, 8, 8, 256
VAMP_RESIZE2D_STRIP_CHUNK, VAMP_RESIZE2D_STRIP_MAX, VAMP_RESIZE2D_MAX_RUN = 256, 1088, 16
VAMP_UPDATE_CHUNK, VAMP_UPDATE_GROWTH_INTERVAL = 4096, 2000
VAMP_UPDATE_PARAM, VAMP_UPDATE_EMA_ONLY = 0, 1
VAMP_UPDATE_SCALE_NONE, VAMP_UPDATE_SCALE_STATIC, VAMP_UPDATE_SCALE_DYNAMIC = 0, 1, 2
VAMP_IMG_MAX_TAPS, VAMP_IMG_TILE_W, VAMP_IMG_TILE_H, VAMP_IMG_FOOT_W, VAMP_IMG_FOOT_H = 16, 64, 8, 272, 48
VAMP_IMG_CONST_COLS, VAMP_IMG_OUT_NONE = 16, -1
VAMP_DET_EVAL_MAX_CLASSES, VAMP_DET_EVAL_GT_CAP, VAMP_DET_EVAL_MAX_WIDTH = 16, 256, 2048
VAMP_DET_EVAL_RECORD_BYTES, VAMP_DET_EVAL_STATE_WORDS = 32, 24
VAMP_DET_EVAL_HALF_PERIOD, VAMP_DET_EVAL_HAS_ORIENT, VAMP_DET_EVAL_HAS_VEL, VAMP_DET_EVAL_HAS_ATTR = 1, 2, 4, 8
VAMP_BN_CHUNK, VAMP_BN_MAX_WORLD = 4096, 64
VAMP_BN_ACT_NONE, VAMP_BN_ACT_RELU = 0, 1
VAMP_ACT_NONE, VAMP_ACT_LEAKY_RELU, VAMP_ACT_SIGMOID = 0, 1, 2
VAMP_CONV_EPI_MAX_SEGS, VAMP_CONV_EPI_CHUNK = 4, 4096


class VampLiftDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32), ("C", C.c_int32),
                ("D", C.c_int32), ("fH", C.c_int32), ("fW", C.c_int32),
                ("Z", C.c_int32), ("Y", C.c_int32), ("X", C.c_int32),
                ("u_max", C.c_float), ("v_max", C.c_float),
                ("u_div", C.c_float), ("v_div", C.c_float),
                ("d_lo", C.c_float), ("d_hi", C.c_float), ("d_span", C.c_float),
                ("use_depth", C.c_int32), ("in_dtype", C.c_int32)]


class VampPoolDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("P", C.c_int64),
                ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("in_dtype", C.c_int32)]


class VampRenderDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("N", C.c_int32),
                ("D", C.c_int32), ("fH", C.c_int32), ("fW", C.c_int32),
                ("K", C.c_int32), ("C", C.c_int32),
                ("Z", C.c_int32), ("Y", C.c_int32), ("X", C.c_int32),
                ("oZ", C.c_int32), ("oY", C.c_int32), ("oX", C.c_int32),
                ("lo", C.c_float * 3), ("span", C.c_float * 3),
                ("d_far", C.c_float), ("z_step_det", C.c_float), ("det_step", C.c_float * 3),
                ("density_mode", C.c_int32), ("sdf_bias", C.c_float), ("beta_min", C.c_float),
                ("cat_seg", C.c_int32), ("in_dtype", C.c_int32)]


class VampConvDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
                ("Z", C.c_int32), ("Y", C.c_int32), ("X", C.c_int32)]


class VampConvEpiSeg(C.Structure):
    """One segment of output channels of a convolution's epilogue (include/vampire_hip.h)."""
    _fields_ = [("bias", C.c_void_p), ("residual", C.c_void_p), ("out", C.c_void_p), ("grad_out", C.c_void_p),
                ("grad_bias", C.c_void_p), ("c0", C.c_int32), ("nch", C.c_int32), ("act", C.c_int32),
                ("out_f32", C.c_int32), ("slope", C.c_float), ("reserved", C.c_int32)]


class VampConvEpilogue(C.Structure):
    _fields_ = [("nseg", C.c_int32), ("reserved", C.c_int32), ("seg", VampConvEpiSeg * VAMP_CONV_EPI_MAX_SEGS)]


class VampSampleDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("C", C.c_int32),
                ("Z", C.c_int32), ("Y", C.c_int32), ("X", C.c_int32),
                ("lo", C.c_float * 3), ("span", C.c_float * 3),
                ("padding", C.c_int32), ("mask_outside", C.c_int32), ("activation", C.c_int32),
                ("density_mode", C.c_int32), ("sdf_bias", C.c_float), ("beta_min", C.c_float),
                ("channel_last_out", C.c_int32), ("in_dtype", C.c_int32), ("lattice", C.c_int32 * 3)]


VAMP_PAD_ZEROS, VAMP_PAD_BORDER = 0, 1


class VampQueryDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("K", C.c_int32),
                ("Z", C.c_int32), ("Y", C.c_int32), ("X", C.c_int32),
                ("lo", C.c_float * 3), ("span", C.c_float * 3),
                ("density_mode", C.c_int32), ("sdf_bias", C.c_float), ("beta_min", C.c_float),
                ("sem_dtype", C.c_int32), ("den_dtype", C.c_int32),
                ("M", C.c_int32), ("want_sdf", C.c_int32), ("P_occ", C.c_int32), ("occ_shared", C.c_int32),
                ("lattice", C.c_int32 * 3)]


class VampConfDesc(C.Structure):
    _fields_ = [("B", C.c_int64), ("S", C.c_int64), ("K", C.c_int32), ("layout", C.c_int32),
                ("pred_dtype", C.c_int32), ("target_dtype", C.c_int32), ("Kc", C.c_int32),
                ("lo", C.c_int32), ("hi", C.c_int32), ("ignore_index", C.c_int32), ("use_ignore", C.c_int32),
                ("reserved", C.c_int32)]


VAMP_NMS_CIRCLE, VAMP_NMS_SIZE_AWARE, VAMP_NMS_ROTATE = 0, 1, 2


class VampDetTask(C.Structure):
    _fields_ = [("heatmap", C.c_void_p), ("reg", C.c_void_p), ("height", C.c_void_p), ("dim", C.c_void_p),
                ("rot", C.c_void_p), ("vel", C.c_void_p)]


class VampDetDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("ncls", C.c_int32 * 8),
                ("max_num", C.c_int32), ("pre_max_size", C.c_int32), ("post_max_size", C.c_int32),
                ("nms_kind", C.c_int32), ("in_dtype", C.c_int32), ("has_vel", C.c_int32), ("norm_bbox", C.c_int32),
                ("use_score_threshold", C.c_int32), ("use_center_range", C.c_int32),
                ("score_threshold", C.c_float), ("out_size_factor", C.c_float), ("voxel_size", C.c_float * 2),
                ("pc_range", C.c_float * 2), ("post_center_range", C.c_float * 6), ("min_radius", C.c_float * 8),
                ("thresh_scale", C.c_float * 8), ("nms_thr", C.c_float * 8), ("reserved", C.c_int32)]


class VampDetTargetDesc(C.Structure):
    _fields_ = [("gaussian_overlap", C.c_double), ("B", C.c_int32), ("T", C.c_int32), ("M", C.c_int32),
                ("ncls", C.c_int32 * 8), ("box_cols", C.c_int32), ("code", C.c_int32), ("max_objs", C.c_int32),
                ("fh", C.c_int32), ("fw", C.c_int32), ("out_size_factor", C.c_int32), ("min_radius", C.c_int32),
                ("norm_bbox", C.c_int32), ("label_dtype", C.c_int32), ("voxel_size", C.c_float * 2),
                ("pc_range", C.c_float * 2), ("reserved", C.c_int32 * 2)]


class VampDetLossDesc(C.Structure):
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("ncls", C.c_int32 * 8),
                ("code", C.c_int32), ("max_objs", C.c_int32), ("has_vel", C.c_int32), ("code_weights", C.c_float * 10),
                ("loss_bbox_weight", C.c_float), ("reserved", C.c_int32 * 2)]


class VampRgbLossDesc(C.Structure):
    _fields_ = [("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("data_range", C.c_float), ("k1", C.c_float), ("k2", C.c_float)]


class VampSegLossDesc(C.Structure):
    _fields_ = [("B", C.c_int64), ("S", C.c_int64), ("C", C.c_int32), ("layout", C.c_int32),
                ("label_dtype", C.c_int32), ("reserved", C.c_int32), ("w_ce", C.c_float), ("w_lv", C.c_float)]


class VampRegTerm(C.Structure):
    _fields_ = [("n", C.c_int64), ("kind", C.c_int32), ("side", C.c_int32), ("pred_dtype", C.c_int32),
                ("target_is_const", C.c_int32), ("target_value", C.c_float), ("reserved", C.c_int32)]


class VampRegLossDesc(C.Structure):
    _fields_ = [("T", C.c_int32), ("reserved", C.c_int32), ("terms", VampRegTerm * VAMP_REG_MAX_TERMS)]


class VampResize2dSeg(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("planes", C.c_int64)]


class VampResize2dDesc(C.Structure):
    _fields_ = [("ih", C.c_int32), ("iw", C.c_int32), ("oh", C.c_int32), ("ow", C.c_int32), ("nseg", C.c_int32),
                ("reserved", C.c_int32), ("seg", VampResize2dSeg * VAMP_RESIZE2D_MAX_SEGS)]


class VampUpdateChunk(C.Structure):
    """One entry of the parameter update's chunk table (device memory; optim.py builds it as a numpy record array)."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("state_off", C.c_int64), ("len", C.c_int32),
                ("kind", C.c_int32)]


class VampUpdateScalars(C.Structure):
    """The parameter update's scalar block (device memory, 128 bytes)."""
    _fields_ = [("lr", C.c_double), ("step", C.c_int64), ("updates", C.c_int64), ("scale", C.c_float),
                ("growth", C.c_int32), ("found_inf", C.c_int32), ("total_norm", C.c_float), ("clip_coef", C.c_float),
                ("mult", C.c_float), ("decay_mul", C.c_float), ("step_size", C.c_float), ("bc2_sqrt", C.c_float),
                ("ema_d", C.c_float), ("ema_1md", C.c_float), ("reserved", C.c_int32 * 15)]


class VampParamUpdateDesc(C.Structure):
    _fields_ = [("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_norm", C.c_double), ("ema_decay", C.c_double), ("n_param_chunks", C.c_int32),
                ("n_buffer_chunks", C.c_int32), ("scale_mode", C.c_int32), ("reserved", C.c_int32)]


class VampLidarLabelDesc(C.Structure):
    _fields_ = [("origin_x", C.c_double), ("origin_y", C.c_double), ("size", C.c_double),
                ("B", C.c_int32), ("N", C.c_int32), ("M", C.c_int32), ("point_cols", C.c_int32),
                ("label_dtype", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("stride", C.c_int32),
                ("raw_w", C.c_int32), ("raw_h", C.c_int32), ("ny", C.c_int32), ("nx", C.c_int32),
                ("z_lo", C.c_float), ("z_hi", C.c_float), ("reserved", C.c_int32 * 2)]


class VampImageDesc(C.Structure):
    _fields_ = [("raw_b_stride", C.c_int64), ("raw_n_stride", C.c_int64), ("raw_row_stride", C.c_int64),
                ("B", C.c_int32), ("N", C.c_int32), ("raw_h", C.c_int32), ("raw_w", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("taps_x", C.c_int32), ("taps_y", C.c_int32),
                ("foot_w", C.c_int32), ("foot_h", C.c_int32), ("out_dtype", C.c_int32), ("to_rgb", C.c_int32),
                ("mean", C.c_float * 3), ("std_inv", C.c_float * 3), ("reserved", C.c_int32 * 2)]


class VampDetEvalDesc(C.Structure):
    _fields_ = [("class_range", C.c_double * VAMP_DET_EVAL_MAX_CLASSES), ("dist_ths", C.c_double * 4),
                ("dist_th_tp", C.c_double), ("B", C.c_int32), ("M", C.c_int32), ("G", C.c_int32),
                ("box_cols", C.c_int32), ("score_dtype", C.c_int32), ("gt_label_dtype", C.c_int32),
                ("has_attrs", C.c_int32), ("num_classes", C.c_int32), ("max_boxes_per_sample", C.c_int32),
                ("max_samples", C.c_int32), ("class_flags", C.c_int32 * VAMP_DET_EVAL_MAX_CLASSES),
                ("attr_moving", C.c_int32 * VAMP_DET_EVAL_MAX_CLASSES),
                ("attr_still", C.c_int32 * VAMP_DET_EVAL_MAX_CLASSES), ("reserved", C.c_int32 * 2)]


class VampBatchNormDesc(C.Structure):
    _fields_ = [("eps", C.c_double), ("momentum", C.c_double), ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("dtype", C.c_int32), ("act", C.c_int32), ("has_residual", C.c_int32),
                ("training", C.c_int32), ("world", C.c_int32), ("update_running", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class VampBevBackwardPlan(C.Structure):
    """What vamp_render_bev_backward_ex will launch (vamp_render_bev_backward_plan; include/vampire_hip.h)."""
    _fields_ = [("scan_lds", C.c_int64), ("path", C.c_int32), ("z_lo", C.c_int32), ("z_hi", C.c_int32),
                ("outside", C.c_int32), ("zero_cam", C.c_int32), ("zero_base", C.c_int32), ("scan", C.c_int32),
                ("scan_grid", C.c_int32 * 3), ("q_grid", C.c_int32 * 3), ("scan_waves", C.c_int32),
                ("raise_lds", C.c_int32), ("beta_parts", C.c_int32), ("fits", C.c_int32), ("nseg", C.c_int32),
                ("zseg", C.c_int32), ("comp_ok", C.c_int32), ("pass_ok", C.c_int32), ("build_table", C.c_int32),
                ("table", C.c_int32), ("comp_body", C.c_int32), ("comp_overwrite", C.c_int32),
                ("seg_gather", C.c_int32), ("base_body", C.c_int32), ("base_overwrite", C.c_int32),
                ("base_body_no_vo", C.c_int32), ("generic", C.c_int32), ("beta_reduce", C.c_int32),
                ("beta_reduce_no_vo", C.c_int32), ("reserved", C.c_int32 * 6)]


class VampCameraForwardPlan(C.Structure):
    """What vamp_render_camera_forward_ex will launch (vamp_render_camera_forward_plan; include/vampire_hip.h)."""
    _fields_ = [("bytes_needed", C.c_int64), ("path", C.c_int32), ("ert", C.c_int32), ("term", C.c_int32),
                ("pack", C.c_int32), ("pack_only", C.c_int32), ("save_rows", C.c_int32), ("body", C.c_int32),
                ("grid", C.c_int32), ("reserved", C.c_int32 * 6)]


class VampCameraBackwardPlan(C.Structure):
    """What vamp_render_camera_backward_acc will launch (vamp_render_camera_backward_plan; include/vampire_hip.h)."""
    _fields_ = [("bytes_needed", C.c_int64), ("ray_lds", C.c_int64), ("path", C.c_int32), ("pack", C.c_int32),
                ("parts", C.c_int32), ("term", C.c_int32), ("samples", C.c_int32), ("prepare", C.c_int32),
                ("ray_cp4", C.c_int32), ("ray_kt", C.c_int32), ("raise_lds", C.c_int32), ("ray_grid", C.c_int32),
                ("list_grid", C.c_int32), ("heavy_grid", C.c_int32), ("heavy_waves", C.c_int32),
                ("gather_grid", C.c_int32), ("accumulate", C.c_int32), ("beta_tail", C.c_int32),
                ("splat_grid", C.c_int32), ("unpack_grid", C.c_int32), ("reserved", C.c_int32 * 6)]


# regions of the render workspace, in layout order (VAMP_RENDERWS_*; "grad" overlays "gcl" .. "beta_part")
RENDERWS_REGIONS = ("packed", "grad", "gcl", "cnt", "off", "bsum", "boff", "aux", "hcells", "part", "runs", "rank",
                    "slot", "tile_se", "tile_order", "records", "beta_part", "term", "rows")


class VampRenderWorkspaceLayout(C.Structure):
    """Byte offset and size of every region of the render workspace (vamp_render_workspace_layout)."""
    _fields_ = [("offset", C.c_int64 * len(RENDERWS_REGIONS)), ("bytes", C.c_int64 * len(RENDERWS_REGIONS)),
                ("base_bytes", C.c_int64), ("bytes_with_rows", C.c_int64)]


class VampLiftForwardPlan(C.Structure):
    """What vamp_lift_forward_ex / vamp_lift_forward_logits_ex will launch (vamp_lift_forward_plan; include/vampire_hip.h)."""
    _fields_ = [("bytes_needed", C.c_int64), ("first", C.c_int32), ("first_grid", C.c_int32), ("sm_tiles", C.c_int32),
                ("sm_reg", C.c_int32), ("ptiles", C.c_int32), ("cull_words", C.c_int32), ("coop", C.c_int32),
                ("ch", C.c_int32), ("emit", C.c_int32), ("counters", C.c_int32), ("scan", C.c_int32),
                ("grid", C.c_int32 * 3), ("reserved", C.c_int32 * 6)]


class VampLiftBackwardPlan(C.Structure):
    """What vamp_lift_backward_ex will launch (vamp_lift_backward_plan; include/vampire_hip.h)."""
    _fields_ = [("bytes_needed", C.c_int64), ("fill_lds", C.c_int64), ("strip_lds", C.c_int64),
                ("zero_feat_bytes", C.c_int64), ("zero_depth_bytes", C.c_int64), ("path", C.c_int32),
                ("feat_cl", C.c_int32), ("prepare", C.c_int32), ("fill_ch", C.c_int32), ("fill_grid", C.c_int32),
                ("cap", C.c_int32), ("raise_lds", C.c_int32), ("vec", C.c_int32), ("strip_grid", C.c_int32),
                ("softmax_bwd", C.c_int32), ("to_cl", C.c_int32), ("splat_ch", C.c_int32),
                ("splat_grid", C.c_int32 * 3), ("to_cf", C.c_int32), ("reserved", C.c_int32 * 6)]


# regions of the lift workspace, in layout order (VAMP_LIFTWS_*)
LIFTWS_REGIONS = ("feat_cl", "gfeat_cl", "cnt", "off", "bsum", "boff", "aux", "amask", "ptaps", "pcell", "recs", "rowq",
                  "cull")


class VampLiftWorkspaceLayout(C.Structure):
    """Byte offset and size of every region of the lift workspace (vamp_lift_workspace_layout)."""
    _fields_ = [("offset", C.c_int64 * len(LIFTWS_REGIONS)), ("bytes", C.c_int64 * len(LIFTWS_REGIONS)),
                ("total_bytes", C.c_int64)]


VAMP_LIFTPLAN_FIRST_NONE, VAMP_LIFTPLAN_FIRST_PROLOGUE, VAMP_LIFTPLAN_FIRST_OPERANDS, VAMP_LIFTPLAN_FIRST_SOFTMAX = 0, 1, 2, 3
VAMP_LIFTPLAN_COUNTERS_NONE, VAMP_LIFTPLAN_COUNTERS_ZERO, VAMP_LIFTPLAN_COUNTERS_CLEAN = 0, 1, 2
VAMP_LIFTPLAN_BWD_CELL, VAMP_LIFTPLAN_BWD_SPLAT = 0, 1
VAMP_CAMPLAN_FWD_DIRECT, VAMP_CAMPLAN_FWD_PLANNED, VAMP_CAMPLAN_FWD_MARCH = 0, 1, 2
VAMP_CAMPLAN_TERM_NONE, VAMP_CAMPLAN_TERM_BUILD, VAMP_CAMPLAN_TERM_CHECK, VAMP_CAMPLAN_TERM_WRITE = 0, 1, 2, 3
VAMP_CAMPLAN_BWD_CELL, VAMP_CAMPLAN_BWD_SPLAT = 0, 1
VAMP_BEVPLAN_PATH_V1, VAMP_BEVPLAN_PATH_NOOP, VAMP_BEVPLAN_PATH_CELL = 0, 1, 2
VAMP_BEVPLAN_SCAN_NONE, VAMP_BEVPLAN_SCAN_QSCAN21, VAMP_BEVPLAN_SCAN_QSCAN0, VAMP_BEVPLAN_SCAN_Q_SCAN = 0, 1, 2, 3
(VAMP_BEVPLAN_BODY_NONE, VAMP_BEVPLAN_BODY_COMP, VAMP_BEVPLAN_BODY_PASS, VAMP_BEVPLAN_BODY_COL,
 VAMP_BEVPLAN_BODY_ZERO) = 0, 1, 2, 3, 4
(VAMP_BEVPLAN_BETA_NONE, VAMP_BEVPLAN_BETA_TAIL_COMP, VAMP_BEVPLAN_BETA_TAIL_BASE, VAMP_BEVPLAN_BETA_LAUNCH,
 VAMP_BEVPLAN_BETA_EARLY) = 0, 1, 2, 3, 4

# flag bits of vamp_lift_backward_ex / vamp_render_camera_backward_acc (include/vampire_hip.h)
VAMP_LIFTFWD_EMIT_PAIRS, VAMP_LIFTFWD_CELLS_CLEAN, VAMP_LIFTFWD_FEAT_CHANNEL_LAST, VAMP_LIFTFWD_DEFER_SCAN = 1, 2, 4, 8
VAMP_LIFTBWD_CELLS_VALID, VAMP_LIFTBWD_SPLAT = 1, 2
VAMP_LIFTBWD_WPP1, VAMP_LIFTBWD_WPP4, VAMP_LIFTBWD_WPP16 = 4, 8, 16
VAMP_LIFTBWD_LOGITS, VAMP_LIFTBWD_FEAT_CHANNEL_LAST = 256, 512
VAMP_CAMBWD_ACCUMULATE, VAMP_CAMBWD_PACKED_VALID, VAMP_CAMBWD_CELLS_VALID, VAMP_CAMBWD_SPLAT = 1, 2, 4, 8
VAMP_CAMBWD_SAMPLES_VALID, VAMP_CAMBWD_TERM_VALID, VAMP_CAMBWD_NO_ERT = 16, 32, 64
VAMP_CAMBWD_PART_RAY, VAMP_CAMBWD_PART_GATHER, VAMP_CAMBWD_PART_HEAVY = 128, 256, 512
VAMP_CAMFWD_SAVE_SAMPLES, VAMP_CAMFWD_NO_ERT, VAMP_CAMFWD_TERM_VALID = 1, 2, 4
VAMP_CAMPREP_TERM_VALID, VAMP_CAMPREP_COUNTERS_CLEAN, VAMP_CAMPREP_RANKED = 1, 4, 8
VAMP_BEVBWD_OVERWRITE_BASE, VAMP_BEVBWD_OVERWRITE_CAM, VAMP_BEVBWD_SAVED_VALID = 1, 2, 4
VAMP_BEVFWD_SAVE, VAMP_BEVFWD_TWO_KERNELS = 1, 2
VAMP_RENDERFWD_SAVE_SAMPLES, VAMP_RENDERFWD_BEV_SAVE, VAMP_RENDERFWD_RANK, VAMP_RENDERFWD_COUNTERS_CLEAN = 1, 2, 4, 8
VAMP_CAMFWD_PACK_ONLY, VAMP_CAMFWD_PACKED_VALID, VAMP_CAMFWD_DIRECT, VAMP_CAMFWD_EXACT_TAPS = 8, 16, 32, 64
VAMP_BEVBWD_ONLY_BASE, VAMP_BEVBWD_SKIP_BASE, VAMP_BEVBWD_TABLE_VALID = 8, 16, 32


_Tensor, _void_p = torch.Tensor, C.c_void_p       # (module globals: from_param runs once per pointer argument of every call)


class TensorPtr(C.c_void_p):
    """`void*` parameter of the signature table: takes a torch tensor (its data_ptr()), None (NULL), an integer address
    or anything c_void_p itself takes (a c_void_p, a ctypes array or pointer).  Contiguity, device and shape are the
    caller's business (ops `_chk`): this type converts, it does not validate."""

    @classmethod
    def from_param(cls, obj):
        if isinstance(obj, _Tensor):
            # a c_void_p, never the bare integer: ctypes passes an int that from_param returns as a 32-bit C int
            return _void_p(obj.data_ptr())
        if obj is None:
            return None
        if isinstance(obj, int):
            return _void_p(obj)
        if isinstance(obj, (str, bytes)):         # (c_void_p would take the characters' address)
            raise TypeError(f"expected a tensor or a pointer, got {type(obj).__name__}")
        return _void_p.from_param(obj)


class _Ret(typing.NamedTuple):
    """What an entry point returns: its ctypes type, and whether that is a VampStatus code (VAMP_OK or negative), which
    the checked set turns into an exception, or a value handed to the caller as it is."""
    ctype: type
    is_status: bool


_STATUS = _Ret(C.c_int, True)
_INT, _SIZE, _STR = _Ret(C.c_int, False), _Ret(C.c_size_t, False), _Ret(C.c_char_p, False)

_P = TensorPtr
_LD = C.POINTER(VampLiftDesc)
_RD = C.POINTER(VampRenderDesc)
_SD = C.POINTER(VampSampleDesc)
_QYD = C.POINTER(VampQueryDesc)
_CD = C.POINTER(VampConvDesc)
_CED = C.POINTER(VampConvEpilogue)
_PD = C.POINTER(VampPoolDesc)
_QD = C.POINTER(VampConfDesc)
_DD = C.POINTER(VampDetDesc)
_TD = C.POINTER(VampDetTargetDesc)
_ED = C.POINTER(VampDetLossDesc)
_TT = C.POINTER(VampDetTask)
_GD = C.POINTER(VampRgbLossDesc)
_SLD = C.POINTER(VampSegLossDesc)
_RLD = C.POINTER(VampRegLossDesc)
_R2D = C.POINTER(VampResize2dDesc)
_PUD = C.POINTER(VampParamUpdateDesc)
_LLD = C.POINTER(VampLidarLabelDesc)
_IMD = C.POINTER(VampImageDesc)
_DED = C.POINTER(VampDetEvalDesc)
_BND = C.POINTER(VampBatchNormDesc)

# name -> (return kind, argtypes); must list every symbol declared in include/vampire_hip.h
SIGNATURES = {
    "vamp_abi_version": (_INT, []),
    "vamp_debug_checks": (_STATUS, [C.c_int]),
    "vamp_last_error": (_STR, []),
    "vamp_profile_enable": (_STATUS, [C.c_int]),
    "vamp_profile_slots": (_INT, []),
    "vamp_profile_select": (_STATUS, [C.c_int]),
    "vamp_profile_read": (_STATUS, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                    C.POINTER(C.c_double)]),
    "vamp_lift_workspace_bytes": (_SIZE, [_LD]),
    "vamp_lift_workspace_layout": (_STATUS, [_LD, C.POINTER(VampLiftWorkspaceLayout)]),
    "vamp_lift_forward_plan": (_STATUS, [_LD, C.c_int, C.c_int32, C.c_int, C.c_size_t, C.POINTER(VampLiftForwardPlan)]),
    "vamp_lift_backward_plan": (_STATUS, [_LD, C.c_int, C.c_size_t, C.POINTER(VampLiftBackwardPlan)]),
    "vamp_lift_forward": (_STATUS, [_LD] + [_P] * 8 + [_P, C.c_size_t, _P]),
    "vamp_lift_forward_logits": (_STATUS, [_LD] + [_P] * 5 + [C.c_int32] + [_P] * 4 + [_P, C.c_size_t, _P]),
    "vamp_lift_forward_ex": (_STATUS, [_LD] + [_P] * 8 + [_P, C.c_size_t, C.c_int, _P]),
    "vamp_lift_forward_logits_ex": (_STATUS, [_LD] + [_P] * 5 + [C.c_int32] + [_P] * 4 + [_P, C.c_size_t, C.c_int, _P]),
    "vamp_lift_backward": (_STATUS, [_LD] + [_P] * 10 + [_P, C.c_size_t, _P]),
    "vamp_lift_backward_ex": (_STATUS, [_LD] + [_P] * 10 + [_P, C.c_size_t, C.c_int, _P]),
    "vamp_lift_prepare": (_STATUS, [_LD] + [_P] * 5 + [_P, C.c_size_t, _P]),
    "vamp_lift_finish_cells": (_STATUS, [_LD, _P, C.c_size_t, _P]),
    "vamp_render_camera_prepare_with_lift": (_STATUS, [_RD] + [_P] * 4 + [_P, C.c_size_t, C.c_int, _LD, _P, C.c_size_t, _P]),
    "vamp_lift_forward_dense": (_STATUS, [_LD] + [_P] * 7 + [_P]),
    "vamp_lift_backward_dense": (_STATUS, [_LD] + [_P] * 7 + [_P]),
    "vamp_lift_indices": (_STATUS, [_LD] + [_P] * 8 + [_P]),
    "vamp_lift_cull_words": (_STATUS, [_LD] + [_P] * 7 + [_P]),
    "vamp_render_workspace_bytes": (_SIZE, [_RD]),
    "vamp_render_camera_forward": (_STATUS, [_RD] + [_P] * 13 + [_P, C.c_size_t, _P]),
    "vamp_render_samples_bytes": (_SIZE, [_RD]),
    "vamp_render_term_offset": (_SIZE, [_RD]),
    "vamp_render_camera_terminate": (_STATUS, [_RD] + [_P] * 6 + [_P, C.c_size_t, _P]),
    "vamp_render_camera_prepare_ex": (_STATUS, [_RD] + [_P] * 4 + [_P, C.c_size_t, C.c_int, _P]),
    "vamp_render_camera_forward_ex": (_STATUS, [_RD] + [_P] * 13 + [_P, C.c_size_t, C.c_int, _P]),
    "vamp_render_camera_backward": (_STATUS, [_RD] + [_P] * 17 + [_P, C.c_size_t, _P]),
    "vamp_render_camera_prepare": (_STATUS, [_RD] + [_P] * 4 + [_P, C.c_size_t, _P]),
    "vamp_render_camera_backward_acc": (_STATUS, [_RD] + [_P] * 17 + [_P, C.c_size_t, C.c_int, _P, _P]),
    "vamp_render_bev_forward": (_STATUS, [_RD] + [_P] * 14 + [_P]),
    "vamp_render_bev_forward_ex": (_STATUS, [_RD] + [_P] * 14 + [C.POINTER(C.c_float), _P, C.c_size_t, C.c_int, _P]),
    "vamp_render_forward_merged_supported": (_INT, [_RD, C.POINTER(C.c_float)]),
    "vamp_render_forward_merged": (_STATUS, [_RD] + [_P] * 8 + [C.POINTER(C.c_float)] + [_P] * 14
                                   + [_P, C.c_size_t, _P, C.c_size_t, _P, C.c_int, _P]),
    "vamp_render_bev_workspace_bytes": (_SIZE, [_RD]),
    "vamp_render_bev_backward": (_STATUS, [_RD] + [_P] * 19 + [C.POINTER(C.c_float), _P, C.c_size_t, _P]),
    "vamp_render_bev_backward_ex": (_STATUS, [_RD] + [_P] * 19 + [C.POINTER(C.c_float), _P, C.c_size_t, C.c_int, _P]),
    "vamp_render_bev_backward_plan": (_STATUS, [_RD, C.POINTER(C.c_float), C.c_int, C.POINTER(VampBevBackwardPlan)]),
    "vamp_render_camera_forward_plan": (_STATUS, [_RD, C.c_int, C.c_int, C.c_size_t, C.POINTER(VampCameraForwardPlan)]),
    "vamp_render_camera_backward_plan": (_STATUS, [_RD, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                                   C.POINTER(VampCameraBackwardPlan)]),
    "vamp_render_workspace_layout": (_STATUS, [_RD, C.POINTER(VampRenderWorkspaceLayout)]),
    "vamp_render_indices": (_STATUS, [_RD] + [_P] * 9 + [_P]),
    "vamp_render_camera_direct_taps": (_STATUS, [_RD] + [_P] * 9 + [_P]),
    "vamp_frustum_geometry": (_STATUS, [_RD] + [_P] * 5 + [_P]),
    "vamp_sample_points_forward": (_STATUS, [_SD, _P, _P, _P, C.c_int64, _P, _P]),
    "vamp_sample_points_workspace_bytes": (_SIZE, [_SD, C.c_int64]),
    "vamp_sample_points_backward": (_STATUS, [_SD, _P, _P, _P, C.c_int64, _P, _P, _P, _P, C.c_size_t, _P]),
    "vamp_point_queries_supported": (_INT, [_QYD]),
    "vamp_point_queries_workspace_bytes": (_SIZE, [_QYD]),
    "vamp_point_queries_forward": (_STATUS, [_QYD] + [_P] * 11),
    "vamp_point_queries_backward": (_STATUS, [_QYD] + [_P] * 13 + [C.c_size_t, _P]),
    "vamp_depth_softmax_forward": (_STATUS, [C.c_int64, C.c_int32, C.c_int64, _P, C.c_int32, _P, _P]),
    "vamp_depth_softmax_backward": (_STATUS, [C.c_int64, C.c_int32, C.c_int64, _P, _P, _P, _P]),
    "vamp_density_gate_forward": (_STATUS, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P, _P]),
    "vamp_upsample_trilinear_forward": (_STATUS, [C.c_int64] + [C.c_int32] * 6 + [_P, _P, _P]),
    "vamp_upsample_trilinear_forward_ex": (_STATUS, [C.c_int64] + [C.c_int32] * 7 + [_P, _P, _P]),
    "vamp_upsample_trilinear_backward_ex": (_STATUS, [C.c_int64] + [C.c_int32] * 7 + [_P, _P, _P, C.c_size_t, _P]),
    "vamp_upsample_trilinear_workspace_bytes": (_SIZE, [C.c_int32] * 3),
    "vamp_upsample_trilinear_supported": (_INT, [C.c_int32] * 6),
    "vamp_upsample_trilinear_backward": (_STATUS, [C.c_int64] + [C.c_int32] * 6 + [_P, _P, _P, C.c_size_t, _P]),
    "vamp_resize2d_supported": (_INT, [C.c_int32] * 4),
    "vamp_resize2d_workspace_bytes": (_SIZE, [C.c_int32] * 4),
    "vamp_resize2d_forward": (_STATUS, [_R2D, _P]),
    "vamp_resize2d_backward": (_STATUS, [_R2D, _P, C.c_size_t, _P]),
    "vamp_conv3d_supported": (_INT, [_CD]),
    "vamp_conv3d_forward": (_STATUS, [_CD, _P, _P, _P, _P]),
    "vamp_conv3d_backward_data": (_STATUS, [_CD, _P, _P, _P, _P]),
    "vamp_conv3d_workspace_bytes": (_SIZE, [_CD]),
    "vamp_conv3d_backward_weight": (_STATUS, [_CD, _P, _P, _P, _P, C.c_size_t, _P]),
    "vamp_conv3d_bf16_supported": (_INT, [_CD]),
    "vamp_conv3d_bf16_forward": (_STATUS, [_CD, _P, _P, _P, _P]),
    "vamp_conv3d_bf16_backward_data": (_STATUS, [_CD, _P, _P, _P, _P]),
    "vamp_conv3d_bf16_workspace_bytes": (_SIZE, [_CD]),
    "vamp_conv3d_bf16_backward_weight": (_STATUS, [_CD, _P, _P, _P, _P, C.c_size_t, _P]),
    "vamp_conv3d_half_forward": (_STATUS, [_CD, C.c_int32, _P, _P, _P, _P]),
    "vamp_conv3d_half_backward_data": (_STATUS, [_CD, C.c_int32, _P, _P, _P, _P]),
    "vamp_conv3d_half_backward_weight": (_STATUS, [_CD, C.c_int32, _P, _P, _P, _P, C.c_size_t, _P]),
    "vamp_conv3d_half_s2_supported": (_INT, [_CD]),
    "vamp_conv3d_half_s2_workspace_bytes": (_SIZE, [_CD]),
    "vamp_conv3d_half_s2_forward": (_STATUS, [_CD, C.c_int32, _P, _P, _P, _P]),
    "vamp_conv3d_half_s2_backward_data": (_STATUS, [_CD, C.c_int32, _P, _P, _P, _P]),
    "vamp_conv3d_half_s2_backward_weight": (_STATUS, [_CD, C.c_int32, _P, _P, _P, _P, C.c_size_t, _P]),
    "vamp_conv3d_epilogue_supported": (_INT, [_CD, C.c_int32, C.c_int32, _CED]),
    "vamp_conv3d_epilogue_forward": (_STATUS, [_CD, _CED, _P, _P, _P]),
    "vamp_conv3d_half_epilogue_forward": (_STATUS, [_CD, C.c_int32, _CED, _P, _P, _P]),
    "vamp_conv3d_half_s2_epilogue_forward": (_STATUS, [_CD, C.c_int32, _CED, _P, _P, _P]),
    "vamp_conv3d_epilogue_workspace_bytes": (_SIZE, [_CD, C.c_int32]),
    "vamp_conv3d_epilogue_backward": (_STATUS, [_CD, C.c_int32, C.c_int32, _CED, _P, _P, C.c_size_t, _P]),
    "vamp_density_gate_backward": (_STATUS, [C.c_int64, C.c_int32, C.c_int64, C.c_int32, _P, _P, _P, _P, _P,
                                             _P]),
    "vamp_voxel_pooling_workspace_bytes": (_SIZE, [_PD]),
    "vamp_voxel_pooling_forward": (_STATUS, [_PD] + [_P] * 3 + [_P, C.c_size_t, _P]),
    "vamp_voxel_pooling_backward": (_STATUS, [_PD] + [_P] * 4),
    "vamp_gate_conv1x1_supported": (_INT, [C.c_int32] * 3),
    "vamp_gate_conv1x1_workspace_bytes": (_SIZE, [C.c_int32] * 3),
    "vamp_gate_conv1x1_forward": (_STATUS, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]
                                  + [_P] * 6),
    "vamp_gate_conv1x1_backward": (_STATUS, [C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32]
                                   + [_P] * 9 + [C.c_size_t, _P]),
    "vamp_confusion_workspace_bytes": (_SIZE, [_QD]),
    "vamp_confusion_update": (_STATUS, [_QD] + [_P] * 5 + [_P, C.c_size_t, _P]),
    "vamp_lidarseg_workspace_bytes": (_SIZE, [C.c_int64, C.c_int64]),
    "vamp_lidarseg_predict": (_STATUS, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int64,
                                        _P, _P, _P, C.c_size_t, _P]),
    "vamp_det_workspace_bytes": (_SIZE, [_DD]),
    "vamp_det_postprocess": (_STATUS, [_DD, C.POINTER(VampDetTask)] + [_P] * 5 + [C.c_size_t, _P]),
    "vamp_det_targets_workspace_bytes": (_SIZE, [_TD]),
    "vamp_det_targets": (_STATUS, [_TD] + [_P] * 7 + [C.c_size_t, _P]),
    "vamp_det_loss_workspace_bytes": (_SIZE, [_ED]),
    "vamp_det_loss_counts": (_STATUS, [_ED, _P, _P, _P, _P]),
    "vamp_det_loss_forward": (_STATUS, [_ED, _TT] + [_P] * 7 + [_P, C.c_size_t, _P]),
    "vamp_det_loss_backward": (_STATUS, [_ED, _TT] + [_P] * 6 + [_TT, _P, C.c_size_t, _P]),
    "vamp_rgb_loss_workspace_bytes": (_SIZE, [_GD]),
    "vamp_rgb_loss_forward": (_STATUS, [_GD] + [_P] * 5 + [_P, C.c_size_t, _P]),
    "vamp_rgb_loss_backward": (_STATUS, [_GD] + [_P] * 4 + [_P, C.c_size_t, _P]),
    "vamp_seg_loss_workspace_bytes": (_SIZE, [_SLD]),
    "vamp_seg_loss_kept_bytes": (_SIZE, [_SLD]),
    "vamp_seg_loss_forward": (_STATUS, [_SLD] + [_P] * 8 + [_P, C.c_size_t, _P, C.c_size_t, _P]),
    "vamp_seg_loss_backward": (_STATUS, [_SLD] + [_P] * 5 + [_P, C.c_size_t, _P]),
    "vamp_reg_loss_workspace_bytes": (_SIZE, [_RLD]),
    "vamp_reg_loss_forward": (_STATUS, [_RLD] + [_P] * 5 + [_P, C.c_size_t, _P]),
    "vamp_reg_loss_backward": (_STATUS, [_RLD] + [_P] * 6 + [_P]),
    "vamp_param_update_workspace_bytes": (_SIZE, [_PUD]),
    "vamp_param_update_step": (_STATUS, [_PUD] + [_P] * 5 + [_P, C.c_size_t, _P]),
    "vamp_lidar_labels_workspace_bytes": (_SIZE, [_LLD]),
    "vamp_lidar_labels": (_STATUS, [_LLD] + [_P] * 12 + [_P, C.c_size_t, _P]),
    "vamp_camera_images_workspace_bytes": (_SIZE, [_IMD]),
    "vamp_camera_images": (_STATUS, [_IMD] + [_P] * 10 + [_P, C.c_size_t, _P]),
    "vamp_det_eval_supported": (_INT, [_DED]),
    "vamp_det_eval_record_bytes": (_SIZE, [_DED]),
    "vamp_det_eval_update": (_STATUS, [_DED] + [_P] * 9 + [_P]),
    "vamp_bn_workspace_bytes": (_SIZE, [_BND]),
    "vamp_bn_partial_stats": (_STATUS, [_BND, _P, _P, _P, C.c_size_t, _P]),
    "vamp_bn_apply": (_STATUS, [_BND] + [_P] * 10 + [_P]),
    "vamp_bn_backward_partial": (_STATUS, [_BND] + [_P] * 7 + [_P, C.c_size_t, _P]),
    "vamp_bn_backward_apply": (_STATUS, [_BND] + [_P] * 9 + [_P]),
}

_lib = None
_checked = None     # (the library it was made from, the checked set)


class VampireHipError(RuntimeError):
    pass


def load():
    """Load the library and bind every symbol; raises if anything is missing.  The functions of the returned library
    hand status codes back as integers (what the C-ABI tests assert on); `checked()` is the set that raises."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("VAMPIRE_HIP_LIB", lib_path())
    if not os.path.exists(path):
        raise VampireHipError(
            f"{path} not found: build it with `python -m vampire_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(path)
    for name, (ret, args) in SIGNATURES.items():
        fn = getattr(lib, name)           # AttributeError if the symbol is missing
        fn.restype = ret.ctype
        fn.argtypes = args
    got = lib.vamp_abi_version()
    if got != ABI_VERSION:
        raise VampireHipError(f"ABI version mismatch: library {got}, binding {ABI_VERSION}")
    _lib = lib
    return lib


def _raise_on_status(last_error, name):
    def errcheck(code, func=None, args=None):
        if code != 0:
            raise VampireHipError(f"{name} failed with code {code}: {last_error().decode('utf-8', 'replace')}")
        return code
    return errcheck


def checked(through=None):
    """The entry points of `load()` once more, as attributes of one object, with every status return checked: a call
    that fails raises VampireHipError with the library's message; the value returns (`*_bytes`, `*_supported`, ...)
    come back as they are.  `through`: a stand-in for the library whose attributes the calls are to go through (the
    tests' call recorders); None or the library itself gives the set bound to the library's own symbols."""
    global _checked
    lib = load()
    if through is not None and through is not lib:
        def via(name):
            fn, check = getattr(through, name), _raise_on_status(lib.vamp_last_error, name)
            return lambda *a: check(fn(*a))
        return types.SimpleNamespace(**{name: via(name) if ret.is_status else getattr(through, name)
                                        for name, (ret, _) in SIGNATURES.items()})
    if _checked is None or _checked[0] is not lib:
        fns = {}
        for name, (ret, args) in SIGNATURES.items():
            fn = lib[name]                # (a function object of its own: lib.name is the unchecked one)
            fn.restype, fn.argtypes = ret.ctype, args
            if ret.is_status:
                fn.errcheck = _raise_on_status(lib.vamp_last_error, name)
            fns[name] = fn
        _checked = (lib, types.SimpleNamespace(**fns))
    return _checked[1]


def profile_enable(on: bool):
    checked().vamp_profile_enable(1 if on else 0)


def profile_select(name=None):
    """Restrict the event timer to one kernel slot (by name); None = all slots."""
    vamp = checked()
    slot = -1
    if name is not None:
        for i in range(vamp.vamp_profile_slots()):
            nm, n, ms = C.c_char_p(), C.c_int(), C.c_double()
            vamp.vamp_profile_read(i, nm, n, ms)
            if nm.value.decode() == name:
                slot = i
        if slot < 0:
            raise KeyError(name)
    vamp.vamp_profile_select(slot)


def profile_read():
    """{kernel name: (launches, total_ms)} since the last profile_enable(True)."""
    vamp = checked()
    out = {}
    for slot in range(vamp.vamp_profile_slots()):
        name, n, ms = C.c_char_p(), C.c_int(), C.c_double()
        vamp.vamp_profile_read(slot, name, n, ms)
        if n.value:
            out[name.value.decode()] = (n.value, ms.value)
    return out
