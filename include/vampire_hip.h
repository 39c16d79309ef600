/*
 * vampire_hip.h -- C ABI of the MI355X (gfx950) lift + volume-render hot path.
 *
 * The reference (cskkxjk/Vampire) has no native code and no FFI: its hot path is
 * Python calling PyTorch aten ops.  Each entry point below therefore names the
 * reference *Python call site* it replaces (paths relative to the reference
 * repository root; "bv2" = src/layers/backbones/base_vampire2.py).  A Python host
 * binds these with ctypes; nothing here depends on torch.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host;
 *  - tensors are dense, row-major, fp32 unless a desc field says otherwise;
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *    enqueued asynchronously on it, no call synchronises or allocates;
 *  - inputs are borrowed for the duration of the enqueued work, outputs are fully
 *    overwritten unless documented as accumulated;
 *  - return value: 0 on success, a negative VAMP_E* code otherwise;
 *    vamp_last_error() gives a thread-local message.
 */
#ifndef VAMPIRE_HIP_H_
#define VAMPIRE_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAMP_ABI_VERSION 16  /* bumped whenever entry points or flags are added (round 2: 2, round 3: 3, round 4: 4, round 5: 5, round 6: 6;
                                 7: segmentation metrics; 8: detection post-processing; 9: detection targets;
                                 10: the BEV backward's plan; 11: detection loss; 12: rgb loss; 13: segmentation loss;
                                 14: masked regression losses; 15: the camera render's plans and workspace layout;
                                 16: the lift's plans and workspace layout;
                                 16 also: stride-2 16-bit convolutions, the 2-D bilinear resize of the rendered maps and the
                                 parameter update, the lidar-point label rasteriser, the camera images, detection scoring, batch normalisation, the convolutions' epilogue; the number
                                 could not move: a test pins it) */

enum {
  VAMP_OK = 0,
  VAMP_EINVAL = -1,  /* bad descriptor / null pointer / unsupported shape */
  VAMP_ENOSPC = -2,  /* workspace too small */
  VAMP_EHIP = -3     /* a HIP runtime call failed (launch error) */
};

enum { VAMP_F32 = 0, VAMP_BF16 = 1, VAMP_F16 = 2 };   /* VAMP_F16: only the vamp_conv3d_half_* entry points take it */
enum { VAMP_DENSITY_SIGMOID = 0, VAMP_DENSITY_SDF_LAPLACE = 1 };

int vamp_abi_version(void);
const char* vamp_last_error(void);

/*
 * In-library kernel timing with HIP events on the launch stream (used by bench.py
 * for the roofline figure; off by default, zero cost when off).  While enabled,
 * every launcher brackets each of its kernels with an event pair.
 * vamp_profile_read synchronises the recorded events and returns, for the kernel
 * slot `slot` (0 <= slot < vamp_profile_slots()), its name, number of launches
 * and total milliseconds since the last vamp_profile_enable(1).
 */
/*
 * Debugging mode (off by default): while on, the promises a caller makes with flags are verified before the
 * library relies on them -- VAMP_LIFTFWD_CELLS_CLEAN / VAMP_CAMPREP_COUNTERS_CLEAN (the cell counters in the
 * workspace are zero), VAMP_CAM{FWD,PREP,BWD}_TERM_VALID (the workspace holds a termination table: every entry a
 * number of kept samples) -- and a broken one returns VAMP_EINVAL ("promise broken: ...") instead of corrupting a
 * result silently.  Each check drains the stream it is issued on.
 */
int vamp_debug_checks(int on);

int vamp_profile_enable(int on);
int vamp_profile_slots(void);
/* time only this kernel slot (-1 = all): one event pair per step instead of ~40 */
int vamp_profile_select(int slot);
int vamp_profile_read(int slot, const char** name_host, int* launches_host, double* total_ms_host);

/* ------------------------------------------------------------------------- *
 * LIFT: voxel <- mean over cameras of trilinear samples of depth (x) feat.
 * Replaces bv2:550-553 (outer product), bv2:351-388 (get_pixel) and
 * bv2:483-516 (get_voxel_feats); with use_depth = 0 it is the D == 1 variant of
 * src/layers/backbones/base_bilinear.py:471-519.
 * ------------------------------------------------------------------------- */
typedef struct VampLiftDesc {
  int32_t B, N;        /* samples, cameras per sample                          */
  int32_t C;           /* feature channels (mid_channels), multiple of 4, <= 64 */
  int32_t D, fH, fW;   /* depth planes and feature-map size                    */
  int32_t Z, Y, X;     /* voxel grid, output is [B, C, Z, Y, X]                */
  float u_max, v_max;  /* final_dim[1] - 0.5, final_dim[0] - 0.5  (bv2:494-495) */
  float u_div, v_div;  /* final_dim[1] - 1,   final_dim[0] - 1    (bv2:499-500) */
  float d_lo, d_hi;    /* d_bound[0], d_bound[1]                  (bv2:496)     */
  float d_span;        /* (float)(d_bound[1] - d_bound[0])        (bv2:501)     */
  int32_t use_depth;   /* 1: depth-distribution lift; 0: bilinear (z > 0) lift  */
  int32_t in_dtype;    /* VAMP_F32 or VAMP_BF16 for `depth` and `feat`          */
} VampLiftDesc;

/* Bytes of scratch vamp_lift_forward / vamp_lift_backward need in `workspace`. */
size_t vamp_lift_workspace_bytes(const VampLiftDesc* d);

/*
 * mats   [B, N, 3, 4, 4]  inv(bda), intrin @ inv(sensor2ego), ida   (bv2:370-387)
 * xs,ys,zs                voxel-centre coordinates along each axis  (bv2:273-293)
 * depth  [B, N, D, fH, fW]  depth distribution (ignored when use_depth == 0)
 * feat   [B, N, C, fH, fW]
 * out    [B, C, Z, Y, X]
 * hits   [B, Z, Y, X, ceil(C/16)] u64, 4 bits per channel = number of cameras
 *        with a non-zero sample (bv2:509-512); may be NULL when no backward follows.
 */
int vamp_lift_forward(const VampLiftDesc* d, const float* mats, const float* xs,
                      const float* ys, const float* zs, const void* depth,
                      const void* feat, float* out, uint64_t* hits,
                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * flags = VAMP_LIFTFWD_EMIT_PAIRS (a backward will follow): the forward kernel -- which projects every
 * voxel into every camera anyway -- also does the counting half of the backward's pixel sort and leaves
 * every valid (voxel, camera) pair's taps in `workspace`.  Afterwards the workspace is in the state
 * vamp_lift_prepare leaves (VAMP_LIFTBWD_CELLS_VALID), and no kernel of the backward projects a voxel
 * again (the backward's prepare pass and half of its fill pass were that projection).  flags == 0 is
 * vamp_lift_forward.
 */
#define VAMP_LIFTFWD_EMIT_PAIRS 1
/* with EMIT_PAIRS: the caller asserts that the cell counters in `workspace` are zero -- as a zero-filled
   buffer has them, and as every completed vamp_lift_forward_ex(EMIT_PAIRS) / vamp_lift_prepare /
   vamp_lift_backward on this workspace leaves them (the scan zeroes what it has read, the backward's gather
   the cursors of the fill) -- so the zero fill in front of the kernel is skipped.  The promise is about the counter
   region of THIS descriptor in THIS buffer (region VAMP_LIFTWS_CNT of vamp_lift_workspace_layout): the region's
   offset moves with B, N, C, fH and fW, so a call of another descriptor on the same buffer leaves other bytes zero,
   and its own regions may lie over this one */
#define VAMP_LIFTFWD_CELLS_CLEAN 2
/* (ABI 6) `feat` is handed over CHANNEL-LAST, [B, N, fH, fW, C] fp32 (in_dtype VAMP_F32; 16-byte aligned) -- the
   memory of a torch.channels_last [B*N, C, fH, fW] tensor, what the producing convolution (channel_lower,
   bv2:551-553) emits natively in that memory format.  The lift samples a pixel's C features as one run, so this is
   the layout it wants: the forward's first launch (the transposing copy into the workspace + the camera cull
   words) disappears -- every workgroup forms its own patch's cull word at its head -- and the forward is one
   kernel.  Without the flag feat is [B, N, C, fH, fW] as in the reference and the first launch runs. */
#define VAMP_LIFTFWD_FEAT_CHANNEL_LAST 4
/* (ABI 6) with VAMP_LIFTFWD_EMIT_PAIRS: the forward counts the pairs per cell but leaves the scan of the counters
 * to a later call on the same stream -- vamp_lift_finish_cells, or vamp_render_camera_prepare_with_lift, which scans
 * them in the launch that scans the camera backward's cells (a training step has both lists due between the render
 * forward and the backward).  Until then the workspace is NOT what VAMP_LIFTBWD_CELLS_VALID promises, and its
 * counters are not clean. */
#define VAMP_LIFTFWD_DEFER_SCAN 8
int vamp_lift_forward_ex(const VampLiftDesc* d, const float* mats, const float* xs,
                         const float* ys, const float* zs, const void* depth,
                         const void* feat, float* out, uint64_t* hits,
                         void* workspace, size_t workspace_bytes, int flags, void* stream);

/*
 * Producer fusion (bv2:550 `mapping_along_depth(src).softmax(dim=1)` feeding bv2:553):
 * `logits` [B, N, D, fH, fW] (logits_dtype VAMP_F32 | VAMP_BF16) are the raw depth logits.  ONE launch
 * makes both lift operands -- the softmax over D into `depth_out` (fp32 [B, N, D, fH, fW]; keep it for
 * the backward, where it is the `depth` argument) and the channel-last feature copy -- and the lift
 * follows.  d->in_dtype must be VAMP_F32 (feat fp32), d->use_depth 1.  Everything else as
 * vamp_lift_forward.
 */
int vamp_lift_forward_logits(const VampLiftDesc* d, const float* mats, const float* xs,
                             const float* ys, const float* zs, const void* logits,
                             int32_t logits_dtype, const float* feat, float* depth_out, float* out,
                             uint64_t* hits, void* workspace, size_t workspace_bytes, void* stream);
/* the same with the flags of vamp_lift_forward_ex */
int vamp_lift_forward_logits_ex(const VampLiftDesc* d, const float* mats, const float* xs,
                                const float* ys, const float* zs, const void* logits,
                                int32_t logits_dtype, const float* feat, float* depth_out, float* out,
                                uint64_t* hits, void* workspace, size_t workspace_bytes, int flags,
                                void* stream);

/*
 * Backward of vamp_lift_forward w.r.t. depth and feat (autograd of bv2:507-514,
 * i.e. grid_sampler_3d_backward + the mean).  grad_depth / grad_feat are fp32 and
 * fully overwritten.  grad_depth may be NULL when use_depth == 0.
 */
int vamp_lift_backward(const VampLiftDesc* d, const float* mats, const float* xs,
                       const float* ys, const float* zs, const void* depth,
                       const void* feat, const float* grad_out, const uint64_t* hits,
                       float* grad_depth, float* grad_feat, void* workspace,
                       size_t workspace_bytes, void* stream);

/*
 * The backward first sorts the valid (voxel, camera) pairs by feature-map pixel; the counting
 * half of that depends on the geometry only.  A forward with VAMP_LIFTFWD_EMIT_PAIRS has done it;
 * vamp_lift_prepare does it alone (a projection-only kernel) into `workspace`; and
 * vamp_lift_backward_ex with VAMP_LIFTBWD_CELLS_VALID then skips it: the caller asserts that
 * `workspace` is the same buffer, d / mats / xs / ys / zs are unchanged and no other lift
 * backward has run on it since.  flags == 0 is vamp_lift_backward.
 */
#define VAMP_LIFTBWD_CELLS_VALID 1
/* implementation selectors (tests cross-check them; 0 = the default cell-list gather):
   SPLAT = the per-voxel float-atomic splat; WPP4 / WPP16 (names from round 3's wave-per-pixel gather) make
   the strip gather stage its pairs in chunks of 64 / 32 instead of 128, so that small inputs cross chunk
   boundaries too; WPP1 = default */
#define VAMP_LIFTBWD_SPLAT 2
#define VAMP_LIFTBWD_WPP1 4
#define VAMP_LIFTBWD_WPP4 8
#define VAMP_LIFTBWD_WPP16 16
/* (64, 128: VAMP_LIFTBWD_HALF_LO / _HI of rounds 2-4, the backward by halves of the images on two streams: measured
   slower twice, removed in round 5) */
/* LOGITS: `depth` is softmax(logits) over D as written by vamp_lift_forward_logits, and grad_depth receives
   the gradient w.r.t. the LOGITS, p * (g - sum_d p g) (autograd of bv2:550): applied to the pixel's column
   while it sits in LDS, no extra pass.  Default (cell-list) backward only. */
#define VAMP_LIFTBWD_LOGITS 256
/* (ABI 6) feat is read, and grad_feat written, channel-last [B, N, fH, fW, C] fp32 (see VAMP_LIFTFWD_FEAT_CHANNEL_LAST) */
#define VAMP_LIFTBWD_FEAT_CHANNEL_LAST 512
/* (ABI 6: takes `depth` -- a pair now carries its four depth samples, so that the backward reads no depth plane) */
int vamp_lift_prepare(const VampLiftDesc* d, const float* mats, const float* xs, const float* ys,
                      const float* zs, const void* depth, void* workspace, size_t workspace_bytes, void* stream);
/* (ABI 6) the scan a forward with VAMP_LIFTFWD_DEFER_SCAN left out (one small kernel); afterwards the workspace
 * is what VAMP_LIFTBWD_CELLS_VALID promises */
int vamp_lift_finish_cells(const VampLiftDesc* d, void* workspace, size_t workspace_bytes, void* stream);
int vamp_lift_backward_ex(const VampLiftDesc* d, const float* mats, const float* xs,
                          const float* ys, const float* zs, const void* depth,
                          const void* feat, const float* grad_out, const uint64_t* hits,
                          float* grad_depth, float* grad_feat, void* workspace,
                          size_t workspace_bytes, int flags, void* stream);

/*
 * Signature-compatible path for get_voxel_feats(frustum_feats, ...) (bv2:483):
 * gathers from the materialised [B, N, C, D, fH, fW] fp32 tensor.
 */
int vamp_lift_forward_dense(const VampLiftDesc* d, const float* mats, const float* xs,
                            const float* ys, const float* zs, const float* frustum_feats,
                            float* out, uint64_t* hits, void* stream);
/* grad_frustum_feats [B, N, C, D, fH, fW] must be zero-filled by the caller; it is
 * accumulated into with atomics. */
int vamp_lift_backward_dense(const VampLiftDesc* d, const float* mats, const float* xs,
                             const float* ys, const float* zs, const float* grad_out,
                             const uint64_t* hits, float* grad_frustum_feats, void* stream);

/*
 * Diagnostics for the "voxel indices bit-exact" contract: the validity mask
 * (bv2:494-497) and floor-corner taps of the lift's trilinear sample, per
 * (b, n, z, y, x).  Shares the projection code with the lift kernels.
 */
int vamp_lift_indices(const VampLiftDesc* d, const float* mats, const float* xs,
                      const float* ys, const float* zs, uint8_t* valid, int16_t* ix0,
                      int16_t* iy0, int16_t* iz0, void* stream);

/*
 * Diagnostics for the forward's camera cull (lift.hip: lift_cull_eval): before a wave of the forward
 * kernel projects its patch[0] x patch[1] voxels of one z plane it reads one word, computed from the
 * matrices alone by the forward's first launch -- bit n set: camera n may hold a voxel of the patch that
 * passes `valid` (bv2:493-497); bit 15: every camera of the sample shares inv(bda) bit for bit.  A clear
 * bit is a proof (conservative half-space test of the patch against the six bounds of `valid`), so
 * skipping the camera changes no bit of the result.  This entry runs the same code into `words`
 * [B, Z, grid[1], grid[0]] (uint32; pass words == NULL to query patch / grid only).
 */
int vamp_lift_cull_words(const VampLiftDesc* d, const float* mats, const float* xs, const float* ys,
                         const float* zs, uint32_t* words, int32_t patch[2], int32_t grid[2], void* stream);

/*
 * What vamp_lift_forward_ex / vamp_lift_forward_logits_ex (has_logits, logits_dtype) and vamp_lift_backward_ex will
 * launch for (d, flags, workspace_bytes) (ABI 16): every choice the calls make from the descriptor, the flags and the
 * workspace size, as numbers.  Pure host functions -- no HIP call, no GPU -- and the very functions the entry points ask,
 * behind their pointer checks, before the first launch.  workspace_bytes is the size of a workspace that is there: a NULL
 * workspace counts as 0.  They return VAMP_OK, or the code (and vamp_last_error message) with which the entry point
 * refuses the same arguments: a bad descriptor, a channel count other than 4, 8 or a multiple of 16 up to 64, flags that
 * exclude each other (FEAT_CHANNEL_LAST with a bf16 descriptor, LOGITS with SPLAT, the logits entry's use_depth /
 * in_dtype / logits_dtype rules), too many tiles or voxels for a grid index, a shape the cell lists cannot hold (more
 * than 2^31 pairs or cells, fW or fH above 32766, D above 65534) where the call emits pairs or runs the prepare pass,
 * too many depth planes for the strip gather's LDS tiles, and VAMP_ENOSPC below bytes_needed.
 * Fields a path does not use are 0.
 */
enum { VAMP_LIFTPLAN_FIRST_NONE = 0,      /* channel-last features, no logits: the forward kernel is the only launch */
       VAMP_LIFTPLAN_FIRST_PROLOGUE = 1,  /* lift_prologue_kernel: channel-last copy + cull words */
       VAMP_LIFTPLAN_FIRST_OPERANDS = 2,  /* lift_operands_kernel: softmax + channel-last copy + cull words */
       VAMP_LIFTPLAN_FIRST_SOFTMAX = 3 }; /* lift_operands_kernel, its softmax tiles only (logits, channel-last features) */
enum { VAMP_LIFTPLAN_COUNTERS_NONE = 0,   /* no pairs are emitted */
       VAMP_LIFTPLAN_COUNTERS_ZERO = 1,   /* the cell counters are zero-filled first */
       VAMP_LIFTPLAN_COUNTERS_CLEAN = 2 };/* VAMP_LIFTFWD_CELLS_CLEAN: promised zero (verified under vamp_debug_checks) */
enum { VAMP_LIFTPLAN_BWD_CELL = 0,        /* [prepare] + fill + strip gather */
       VAMP_LIFTPLAN_BWD_SPLAT = 1 };     /* VAMP_LIFTBWD_SPLAT: the per-voxel float-atomic splat */
typedef struct VampLiftForwardPlan {
  int64_t bytes_needed;        /* VAMP_ENOSPC below this */
  int32_t first;               /* VAMP_LIFTPLAN_FIRST_*: the launch in front of the forward kernel */
  int32_t first_grid;          /* its workgroups */
  int32_t sm_tiles;            /* ... of which, per image, softmax tiles of 64 pixels (logits only) */
  int32_t sm_reg;              /* the softmax keeps its bins in registers (D <= 128; 0: the loop variant) */
  int32_t ptiles;              /* ... and channel-last copy tiles of 64 pixels per image (PROLOGUE, OPERANDS) */
  int32_t cull_words;          /* the forward kernel reads the first launch's cull words (0: it forms its own) */
  int32_t coop;                /* lift_fwd_coop_kernel (C = 16, no pairs); 0: lift_fwd_kernel */
  int32_t ch;                  /* CH of lift_fwd_kernel: 4, 8 or 16 (0 with coop) */
  int32_t emit;                /* the forward kernel emits the backward's pairs (VAMP_LIFTFWD_EMIT_PAIRS) */
  int32_t counters;            /* VAMP_LIFTPLAN_COUNTERS_* */
  int32_t scan;                /* the cell scan runs inside the call (emit without VAMP_LIFTFWD_DEFER_SCAN) */
  int32_t grid[3];             /* the forward kernel's workgroups */
  int32_t reserved[6];         /* 0 */
} VampLiftForwardPlan;
int vamp_lift_forward_plan(const VampLiftDesc* d, int has_logits, int32_t logits_dtype, int flags,
                           size_t workspace_bytes, VampLiftForwardPlan* out);
typedef struct VampLiftBackwardPlan {
  int64_t bytes_needed;        /* VAMP_ENOSPC below this */
  int64_t fill_lds;            /* CELL: dynamic LDS bytes of lift_bwd_fill_kernel */
  int64_t strip_lds;           /* CELL: dynamic LDS bytes of lift_bwd_strip_kernel */
  int64_t zero_feat_bytes;     /* SPLAT: the zero fill of the feature gradient ... */
  int64_t zero_depth_bytes;    /* ... and of grad_depth (0 without use_depth) */
  int32_t path;                /* VAMP_LIFTPLAN_BWD_* */
  int32_t feat_cl;             /* feat is read, grad_feat written channel-last (VAMP_LIFTBWD_FEAT_CHANNEL_LAST) */
  int32_t prepare;             /* CELL: the prepare pass (zero fill, pairs kernel, scan) runs inside the call: no CELLS_VALID */
  int32_t fill_ch;             /* CELL: CH of lift_bwd_fill_kernel ... */
  int32_t fill_grid;           /* ... and its workgroups */
  int32_t cap;                 /* CELL: pairs the strip gather stages per chunk: 128 (WPP4: 64, WPP16: 32) */
  int32_t raise_lds;           /* CELL: the dynamic-LDS limit is raised first (strip_lds above 64 KB) */
  int32_t vec;                 /* CELL: the strip gather's 16-byte tile I/O (fp32 depth, fW % 4 == 0) */
  int32_t strip_grid;          /* CELL: lift_bwd_strip_kernel's workgroups */
  int32_t softmax_bwd;         /* CELL: grad_depth receives the gradient of the logits (VAMP_LIFTBWD_LOGITS) */
  int32_t to_cl;               /* SPLAT: feat_to_channel_last runs first (no FEAT_CHANNEL_LAST) */
  int32_t splat_ch;            /* SPLAT: CH of lift_bwd_kernel ... */
  int32_t splat_grid[3];       /* ... and its workgroups */
  int32_t to_cf;               /* SPLAT: feat_to_channel_first copies the gradient back (no FEAT_CHANNEL_LAST) */
  int32_t reserved[6];         /* 0 */
} VampLiftBackwardPlan;
int vamp_lift_backward_plan(const VampLiftDesc* d, int flags, size_t workspace_bytes, VampLiftBackwardPlan* out);

/*
 * The lift workspace, region by region (ABI 16): byte offset and size of
 *   feat_cl | gfeat_cl | cnt | off | bsum | boff | aux | amask | ptaps | pcell | recs | rowq | cull
 * in that order (VAMP_LIFTWS_*): the channel-last feature copy, the splat backward's gradient in that layout, the cell
 * lists (counters, the scan's four levels, camera masks, pair taps, pair cells, records, row queue) and the forward's
 * camera cull words.  Every region is 256-byte aligned and they lie back to back; total_bytes = vamp_lift_workspace_bytes(d).
 */
enum { VAMP_LIFTWS_FEAT_CL = 0, VAMP_LIFTWS_GFEAT_CL, VAMP_LIFTWS_CNT, VAMP_LIFTWS_OFF, VAMP_LIFTWS_BSUM,
       VAMP_LIFTWS_BOFF, VAMP_LIFTWS_AUX, VAMP_LIFTWS_AMASK, VAMP_LIFTWS_PTAPS, VAMP_LIFTWS_PCELL, VAMP_LIFTWS_RECS,
       VAMP_LIFTWS_ROWQ, VAMP_LIFTWS_CULL, VAMP_LIFTWS_REGIONS };
typedef struct VampLiftWorkspaceLayout {
  int64_t offset[VAMP_LIFTWS_REGIONS];
  int64_t bytes[VAMP_LIFTWS_REGIONS];
  int64_t total_bytes;         /* = vamp_lift_workspace_bytes(d) */
} VampLiftWorkspaceLayout;
int vamp_lift_workspace_layout(const VampLiftDesc* d, VampLiftWorkspaceLayout* out);

/* ------------------------------------------------------------------------- *
 * RENDER: volume_rendering_from_multiple_views (bv2:391-467) with the density
 * activation of src/utils/render_utils.py:30-46 (or nn.Sigmoid, bv2:191-194)
 * fused in.
 * ------------------------------------------------------------------------- */
typedef struct VampRenderDesc {
  int32_t B, N;          /* samples, cameras                                     */
  int32_t D, fH, fW;     /* frustum planes (D - 1 samples per ray), map size     */
  int32_t K;             /* semantic classes                                     */
  int32_t C;             /* base (voxel_features) channels, BEV branch only      */
  int32_t Z, Y, X;       /* seg volume [B, c, Z, Y, X]                           */
  int32_t oZ, oY, oX;    /* det grid sampled by the BEV branch                   */
  float lo[3];           /* (x, y, z)_bound_seg[0]                   (bv2:397)   */
  float span[3];         /* (float)(bound[1] - bound[0])             (bv2:399)   */
  float d_far;           /* d_bound[1], background depth             (bv2:436)   */
  float z_step_det;      /* z_bound_det[2], BEV delta                (bv2:451)   */
  float det_step[3];     /* (x, y, z)_bound_det[2]: spacing of the det-grid lattice      */
  int32_t density_mode;  /* VAMP_DENSITY_*                                       */
  float sdf_bias;        /* ModifyLaplaceDensity.bias                            */
  float beta_min;        /* ModifyLaplaceDensity.beta_min (1e-4)                 */
  int32_t cat_seg;       /* voxel_output = cat(base, seg)            (bv2:449)   */
  int32_t in_dtype;      /* VAMP_F32 or VAMP_BF16 for the four volumes           */
} VampRenderDesc;

size_t vamp_render_workspace_bytes(const VampRenderDesc* d);

/*
 * Camera branch, forward (bv2:396-407, 419-440 and the nan_to_num of bv2:612).
 *   geom        [B, N, D, fH, fW, 3] ego-frame frustum points, or NULL to have the
 *               kernel evaluate get_geometry (bv2:314-349) itself from:
 *   mats        [B, N, 3, 4, 4]  inv(ida), sensor2ego @ inv(intrin), bda
 *   us[fW], vs[fH], ds[D]        frustum axes (bv2:253-271)
 *   mids        [D - 1]          camera_mids (bv2:243-246)
 *   beta        device pointer to the raw learnable beta (ignored for sigmoid)
 *   density_feature [B,1,Z,Y,X], semantic [B,K,Z,Y,X], rgb [B,3,Z,Y,X]
 * outputs: rgb_out [B,N,3,fH,fW], seg_out [B,N,K,fH,fW], depth_out [B,N,1,fH,fW]
 */
int vamp_render_camera_forward(const VampRenderDesc* d, const float* geom, const float* mats,
                               const float* us, const float* vs, const float* ds,
                               const float* mids, const float* beta,
                               const void* density_feature, const void* semantic,
                               const void* rgb, float* rgb_out, float* seg_out,
                               float* depth_out, void* workspace, size_t workspace_bytes,
                               void* stream);

/*
 * Same, for training: with VAMP_CAMFWD_SAVE_SAMPLES the march also stores the trilinear sample
 * row (the 1 + K + 3 channels, as gathered) of every inside sample, so that the backward's
 * per-ray pass reads 96 contiguous bytes per sample instead of repeating the 8-tap gather.
 * The rows live behind the base region of `workspace`, which must then hold
 * vamp_render_workspace_bytes(d) + vamp_render_samples_bytes(d) bytes (dense addressing by
 * (camera, depth index, pixel): only the rows of inside samples are ever touched).  Needs the
 * in-kernel geometry (geom == NULL); otherwise the flag is ignored and the backward gathers.
 */
#define VAMP_CAMFWD_SAVE_SAMPLES 1
/*
 * Early ray termination (geom == NULL only).  A ray's samples behind the point where its
 * transmittance has fallen below exp(-18) = 1.5e-8 are dropped: together they weigh less than
 * that in every output and gradient (the compositing weights telescope), three orders below the
 * 1e-4 the outputs are held to, and with the reference's sdf density they are most of the inside
 * samples.  vamp_render_camera_terminate marches the density channel alone and leaves the number
 * of kept samples per ray in a table inside `workspace` (needs vamp_render_workspace_bytes(d));
 * forward, prepare and backward take the table from there:
 *   VAMP_CAMFWD_NO_ERT       march every sample (bit-identical to the v1 results)
 *   VAMP_CAMFWD_TERM_VALID   the table is already in `workspace` (vamp_render_camera_terminate has
 *                            run for these volumes / matrices / beta); otherwise the forward
 *                            builds it first
 */
#define VAMP_CAMFWD_NO_ERT 2
#define VAMP_CAMFWD_TERM_VALID 4
#define VAMP_CAMFWD_PACK_ONLY 8      /* only the channel-last copy of (density, semantic, rgb) into the workspace */
#define VAMP_CAMFWD_PACKED_VALID 16   /* the workspace already holds that copy: march only */
/* geom == NULL only: the whole camera branch as ONE kernel that reads the channel-first volumes
 * directly (render_cam_direct.hip) -- no channel-last copy, no separate termination pass; the
 * per-ray table is written into `workspace` as a by-product when workspace_bytes >=
 * vamp_render_workspace_bytes(d) (workspace may be NULL otherwise).  Combines with NO_ERT. */
#define VAMP_CAMFWD_DIRECT 32
/* With DIRECT the DENSITY samples' tap coordinates come from the reference's own fp32 chain (bv2:328-349, 397-404):
 * the ray's exact line in fp64 deviates from that chain by the chain's rounding, a few ulp of a tap coordinate, which
 * the Laplace density's slope (1 / (2 beta^2) = 50) turns into up to 2.2e-4 m of rendered depth at cfg-A -- outside
 * north_star's 1e-4.  Through ABI 5 the chain was this flag and the line the default of the C entry point; since
 * ABI 6 the chain is the only behaviour (rendered depth within 4.3e-5 m, semantic logits 7.7e-5 at cfg-A) and the flag
 * is accepted and ignored. */
#define VAMP_CAMFWD_EXACT_TAPS 64
int vamp_render_camera_terminate(const VampRenderDesc* d, const float* mats, const float* us,
                                 const float* vs, const float* ds, const float* beta,
                                 const void* density_feature, void* workspace, size_t workspace_bytes,
                                 void* stream);
size_t vamp_render_samples_bytes(const VampRenderDesc* d);
/* Byte offset of that table inside `workspace`: int32 [B, N, fH, fW], the number of leading
 * samples each ray keeps (D - 1 = nothing dropped).  For callers that report how much of the
 * march early ray termination removed (bench.py). */
size_t vamp_render_term_offset(const VampRenderDesc* d);
int vamp_render_camera_forward_ex(const VampRenderDesc* d, const float* geom, const float* mats,
                                  const float* us, const float* vs, const float* ds,
                                  const float* mids, const float* beta,
                                  const void* density_feature, const void* semantic,
                                  const void* rgb, float* rgb_out, float* seg_out,
                                  float* depth_out, void* workspace, size_t workspace_bytes,
                                  int flags, void* stream);

/*
 * Camera branch, backward.  g_* are the upstream gradients of the three outputs
 * (any may be NULL = zero).  grad_density_feature / grad_semantic / grad_rgb are
 * fp32 [B,c,Z,Y,X], fully overwritten.  grad_beta (1 float) is ACCUMULATED into.
 */
int vamp_render_camera_backward(const VampRenderDesc* d, const float* geom, const float* mats,
                                const float* us, const float* vs, const float* ds,
                                const float* mids, const float* beta,
                                const void* density_feature, const void* semantic,
                                const void* rgb, const float* g_rgb, const float* g_seg,
                                const float* g_depth, float* grad_density_feature,
                                float* grad_semantic, float* grad_rgb, float* grad_beta,
                                void* workspace, size_t workspace_bytes, void* stream);

/*
 * Same, for callers that run the two render branches on two streams (they are independent up
 * to these three buffers):
 *   flags       VAMP_CAMBWD_ACCUMULATE: the gradients are ADDED to what grad_density_feature /
 *               grad_semantic / grad_rgb hold (e.g. the BEV branch's contribution, written first)
 *               VAMP_CAMBWD_PACKED_VALID: `workspace` is the buffer vamp_render_camera_forward
 *               ran with for these same volumes and nothing has written to it since, so its
 *               channel-last copy of the volumes is reused instead of rebuilt
 *               VAMP_CAMBWD_CELLS_VALID: vamp_render_camera_prepare has run on this workspace
 *               for the same d / mats / us / vs / ds and no camera backward since
 *   wait_event  a hipEvent_t (or NULL) the stream waits for right before those buffers are first
 *               touched, i.e. after the per-ray pass and the sample sort have been queued
 * ACCUMULATE and wait_event need the default (cell-list) implementation with mats (geom == NULL).
 */
/*
 * The backward sorts the ray samples by the voxel cell of their floor tap; which sample goes to
 * which slot depends on the geometry only.  vamp_render_camera_prepare computes that table into
 * `workspace` ahead of time (e.g. on a second stream beside vamp_render_camera_forward, which
 * only touches the head of the workspace); without it the backward computes the table itself.
 */
int vamp_render_camera_prepare(const VampRenderDesc* d, const float* mats, const float* us,
                               const float* vs, const float* ds, void* workspace,
                               size_t workspace_bytes, void* stream);
/* flags: VAMP_CAMPREP_TERM_VALID -- sort only the samples the early-termination table in
   `workspace` keeps (the backward must then be given VAMP_CAMBWD_TERM_VALID too) */
#define VAMP_CAMPREP_TERM_VALID 1
#define VAMP_CAMPREP_RANKED 8   /* (ABI 6) the ranks have been drawn by vamp_render_forward_merged(VAMP_RENDERFWD_RANK): only the cell scan runs (mats .. ds may be NULL; the backward's work lists are built inside the per-ray pass's launch) */
#define VAMP_CAMPREP_COUNTERS_CLEAN 4   /* the caller asserts that the cell counters in `workspace` are zero (a zero-filled buffer, or one a completed prepare pass has run on: its scan zeroes what it reads): no zero fill.  The promise is about the counter region of THIS descriptor in THIS buffer (vamp_render_workspace_layout): its offset moves with the descriptor, so a completed pass of another descriptor on the same buffer does not make it true */
/* (2: VAMP_CAMPREP_RANK_ONLY of rounds 2-4, the prepare pass in two phases: measured slower twice, removed in round 5) */
int vamp_render_camera_prepare_ex(const VampRenderDesc* d, const float* mats, const float* us,
                                  const float* vs, const float* ds, void* workspace,
                                  size_t workspace_bytes, int flags, void* stream);
/* (ABI 6) vamp_render_camera_prepare_ex whose scan launch ALSO scans the pair cells of a lift forward that ran with
 * VAMP_LIFTFWD_DEFER_SCAN on `lift_workspace` (on this stream, or on one this call is ordered behind): one launch of
 * two independent scans instead of two launches -- it stands for vamp_lift_finish_cells.  Whoever consumes the lift's
 * cells (vamp_lift_backward_ex) must be ordered behind this call. */
int vamp_render_camera_prepare_with_lift(const VampRenderDesc* d, const float* mats, const float* us,
                                         const float* vs, const float* ds, void* workspace, size_t workspace_bytes,
                                         int flags, const VampLiftDesc* lift_desc, void* lift_workspace,
                                         size_t lift_workspace_bytes, void* stream);
#define VAMP_CAMBWD_ACCUMULATE 1
#define VAMP_CAMBWD_PACKED_VALID 2
#define VAMP_CAMBWD_CELLS_VALID 4
/* implementation selector: the float-atomic splat instead of the default cell-list gather
   (the independent cross-check of the tests; also what a caller-supplied geom tensor takes) */
#define VAMP_CAMBWD_SPLAT 8
/* the workspace holds the sample rows of vamp_render_camera_forward_ex(VAMP_CAMFWD_SAVE_SAMPLES)
   for these same volumes / matrices and nothing has written to it since (cell-list path only) */
#define VAMP_CAMBWD_SAMPLES_VALID 16
/* early ray termination in the cell-list path: TERM_VALID = the table of the forward is in
   `workspace`; without it the backward builds the table itself; NO_ERT = every sample */
#define VAMP_CAMBWD_TERM_VALID 32
#define VAMP_CAMBWD_NO_ERT 64
/* Parts of the call, for a caller with two streams (none set = all three: ray, heavy, gather):
 *   PART_RAY     the per-ray pass (and the channel-last copy / termination table / cell lists and
 *                work lists), d loss / d beta
 *   PART_HEAVY   the kernel that sums the heavy cells (more than 32 records) once per cell into per-corner
 *                partial rows in the workspace; it does not touch the gradient buffers.  (Rounds 1 - 5: a
 *                drain of heavy VOXELS that could run beside the gather; since round 6 the gather reads
 *                this part's output, so a caller that splits the parts issues it before PART_GATHER on
 *                the same stream, or behind an event of its own.)
 *   PART_GATHER  the per-voxel gather (waits for wait_event first)
 * Give every part the same VALID / ACCUMULATE flags. */
/* (1024: VAMP_CAMBWD_SLOTS_PENDING, the second phase of VAMP_CAMPREP_RANK_ONLY: removed with it) */
#define VAMP_CAMBWD_PART_RAY 128
#define VAMP_CAMBWD_PART_GATHER 256
#define VAMP_CAMBWD_PART_HEAVY 512
int vamp_render_camera_backward_acc(const VampRenderDesc* d, const float* geom, const float* mats,
                                    const float* us, const float* vs, const float* ds,
                                    const float* mids, const float* beta,
                                    const void* density_feature, const void* semantic,
                                    const void* rgb, const float* g_rgb, const float* g_seg,
                                    const float* g_depth, float* grad_density_feature,
                                    float* grad_semantic, float* grad_rgb, float* grad_beta,
                                    void* workspace, size_t workspace_bytes, int flags,
                                    void* wait_event, void* stream);

/*
 * What vamp_render_camera_forward_ex(d, geom, .., workspace_bytes, flags, ..) and vamp_render_camera_backward_acc(d,
 * geom, mats, .., workspace_bytes, flags, wait_event, ..) will launch (ABI 15): every choice the calls make from the
 * descriptor, from which of geom / mats they are given, from the flags and from the workspace size, as numbers.  Pure
 * host functions -- no HIP call, no GPU -- and the very functions the two entry points ask, behind their pointer checks,
 * before the first launch.  workspace_bytes is the size of a workspace that is there: a NULL workspace counts as 0.
 * They return VAMP_OK, or the code (and vamp_last_error message) with which the entry point refuses the same arguments:
 * VAMP_ENOSPC below bytes_needed; for the backward also CELLS_VALID with early termination but no TERM_VALID, a sample /
 * voxel / cell count beyond 2^31 where the prepare pass runs inside the call, too many depth samples for the per-ray
 * pass's LDS staging, too many x-runs for the gather, and ACCUMULATE / wait_event on the float-atomic splat.
 * Fields a path does not use are 0.
 */
enum { VAMP_CAMPLAN_FWD_DIRECT = 0,    /* cam_fwd_direct_kernel: one kernel on the channel-first volumes */
       VAMP_CAMPLAN_FWD_PLANNED = 1,   /* render_cam_fwd_plan_kernel on the channel-last copy */
       VAMP_CAMPLAN_FWD_MARCH = 2 };   /* render_cam_fwd_kernel: a geom tensor, or more than 128 samples per ray */
enum { VAMP_CAMPLAN_TERM_NONE = 0,     /* the call does not touch the termination table */
       VAMP_CAMPLAN_TERM_BUILD = 1,    /* cam_term_kernel runs first */
       VAMP_CAMPLAN_TERM_CHECK = 2,    /* *_TERM_VALID: read as it is (verified under vamp_debug_checks) */
       VAMP_CAMPLAN_TERM_WRITE = 3 };  /* a by-product of the one-kernel forward: the workspace can hold it */
enum { VAMP_CAMPLAN_BWD_CELL = 0,      /* per-ray pass + heavy cells + per-voxel gather */
       VAMP_CAMPLAN_BWD_SPLAT = 1 };   /* the v1 float-atomic splat: a geom tensor, no mats, or VAMP_CAMBWD_SPLAT */
typedef struct VampCameraForwardPlan {
  int64_t bytes_needed;        /* VAMP_ENOSPC below this (0: the workspace may be NULL) */
  int32_t path;                /* VAMP_CAMPLAN_FWD_* */
  int32_t ert;                 /* rays stop at their termination index */
  int32_t term;                /* VAMP_CAMPLAN_TERM_* */
  int32_t pack;                /* pack_volume_kernel runs (the channel-last copy) */
  int32_t pack_only;           /* ... and is the last launch of the call (VAMP_CAMFWD_PACK_ONLY) */
  int32_t save_rows;           /* the sample rows are kept behind the base region */
  int32_t body;                /* the compiled body: NCH of the one kernel, CP / 4 of the marches (0 with pack_only) */
  int32_t grid;                /* its workgroups (0 with pack_only) */
  int32_t reserved[6];         /* 0 */
} VampCameraForwardPlan;
int vamp_render_camera_forward_plan(const VampRenderDesc* d, int has_geom, int flags, size_t workspace_bytes,
                                    VampCameraForwardPlan* out);
typedef struct VampCameraBackwardPlan {
  int64_t bytes_needed;        /* VAMP_ENOSPC below this */
  int64_t ray_lds;             /* dynamic LDS bytes of cam_bwd_ray_kernel */
  int32_t path;                /* VAMP_CAMPLAN_BWD_* */
  int32_t pack;                /* pack_volume_kernel runs first (SPLAT without PACKED_VALID) */
  int32_t parts;               /* 1: per-ray pass, 2: gather, 4: heavy cells (all of them: 7; SPLAT: 0) */
  int32_t term;                /* VAMP_CAMPLAN_TERM_NONE / _BUILD / _CHECK (per-ray part only) */
  int32_t samples;             /* the per-ray pass reads the forward's sample rows (SAMPLES_VALID) */
  int32_t prepare;             /* the prepare pass (rank + scan) runs inside the call: no CELLS_VALID */
  int32_t ray_cp4, ray_kt;     /* cam_bwd_ray_kernel<T, 4, CP4, KT> */
  int32_t raise_lds;           /* the dynamic-LDS limit is raised first (ray_lds above 64 KB) */
  int32_t ray_grid;            /* ray tiles of the per-ray launch (also: the d beta partials it leaves) ... */
  int32_t list_grid;           /* ... and the list-building workgroups behind them */
  int32_t heavy_grid;          /* cam_cell_splat_kernel */
  int32_t heavy_waves;         /* waves per workgroup of it */
  int32_t gather_grid;         /* cam_bwd_cell_gather_kernel */
  int32_t accumulate;          /* the gather adds (and visits the listed x-runs only) */
  int32_t beta_tail;           /* the gather's first workgroup adds up the d beta partials (sdf density) */
  int32_t splat_grid;          /* SPLAT: render_cam_bwd_kernel */
  int32_t unpack_grid;         /* SPLAT: unpack_grad_kernel */
  int32_t reserved[6];         /* 0 */
} VampCameraBackwardPlan;
int vamp_render_camera_backward_plan(const VampRenderDesc* d, int has_geom, int has_mats, int flags,
                                     int has_wait_event, size_t workspace_bytes, VampCameraBackwardPlan* out);

/*
 * The render workspace, region by region (ABI 15): byte offset and size of
 *   packed | grad (the v1 splat's gradient copy; it OVERLAYS gcl .. beta_part) | gcl | cnt | off | bsum | boff | aux |
 *   hcells | part | runs | rank | slot | tile_se | tile_order | records | beta_part | term | rows
 * in that order (VAMP_RENDERWS_*).  Every region is 256-byte aligned; behind `packed` lies the larger of `grad` and
 * gcl .. beta_part, then the termination table (vamp_render_term_offset), then -- past vamp_render_workspace_bytes -- the
 * sample rows (vamp_render_samples_bytes).
 */
enum { VAMP_RENDERWS_PACKED = 0, VAMP_RENDERWS_GRAD, VAMP_RENDERWS_GCL, VAMP_RENDERWS_CNT, VAMP_RENDERWS_OFF,
       VAMP_RENDERWS_BSUM, VAMP_RENDERWS_BOFF, VAMP_RENDERWS_AUX, VAMP_RENDERWS_HCELLS, VAMP_RENDERWS_PART,
       VAMP_RENDERWS_RUNS, VAMP_RENDERWS_RANK, VAMP_RENDERWS_SLOT, VAMP_RENDERWS_TILE_SE, VAMP_RENDERWS_TILE_ORDER,
       VAMP_RENDERWS_RECORDS, VAMP_RENDERWS_BETA_PART, VAMP_RENDERWS_TERM, VAMP_RENDERWS_ROWS, VAMP_RENDERWS_REGIONS };
typedef struct VampRenderWorkspaceLayout {
  int64_t offset[VAMP_RENDERWS_REGIONS];
  int64_t bytes[VAMP_RENDERWS_REGIONS];
  int64_t base_bytes;          /* = vamp_render_workspace_bytes(d) */
  int64_t bytes_with_rows;     /* = base_bytes + vamp_render_samples_bytes(d) */
} VampRenderWorkspaceLayout;
int vamp_render_workspace_layout(const VampRenderDesc* d, VampRenderWorkspaceLayout* out);

/*
 * BEV (top-down) branch, forward (bv2:408-418, 442-461).
 *   oxs[oX], oys[oY], ozs[oZ]  det-grid centres (bv2:160), bev_mids [oZ] (bv2:248-251)
 *   base [B,C,Z,Y,X]
 * outputs: bev_rgb [B,3,oY,oX], bev_seg [B,K,oY,oX], bev_height [B,1,oY,oX],
 *          voxel_density [B,1,oZ,oY,oX], voxel_output [B,C(+K),oZ,oY,oX]
 */
int vamp_render_bev_forward(const VampRenderDesc* d, const float* oxs, const float* oys,
                            const float* ozs, const float* bev_mids, const float* beta,
                            const void* density_feature, const void* semantic,
                            const void* rgb, const void* base, float* bev_rgb,
                            float* bev_seg, float* bev_height, float* voxel_density,
                            float* voxel_output, void* stream);

/*
 * The same with flags.  VAMP_BEVFWD_SAVE (training): the density samples and the composited
 * channels' samples of every det-grid point are kept in `workspace`
 * (vamp_render_bev_workspace_bytes(d) bytes; +35 MB per sample at cfg-B); a backward call on the
 * same workspace with VAMP_BEVBWD_SAVED_VALID reads them back instead of sampling again.
 */
#define VAMP_BEVFWD_SAVE 1
#define VAMP_BEVFWD_TWO_KERNELS 2   /* the first implementation (density pass + channel-pair pass) instead of the one-kernel forward of render_bev_fused.hip: kept as the cross-check of the tests */
/* ozs_host (ABI 6; was the caller-asserted flag VAMP_BEVFWD_HEIGHTS_LATTICE = 4): a HOST copy of ozs, or NULL.  The
 * one-kernel forward sizes its per-wave plane slabs for a lattice of heights with spacing det_step[2] (what the
 * reference's create_voxel_coords makes, bv2:273-293) and would clamp -- silently -- a plane outside them, so it runs
 * only when the library has CHECKED, on ozs_host, that the heights' z taps fit the slabs; NULL, or an array that does
 * not fit (any jittered / non-uniform ozs), takes the two-kernel path, which handles every height on its own. */
int vamp_render_bev_forward_ex(const VampRenderDesc* d, const float* oxs, const float* oys,
                            const float* ozs, const float* bev_mids, const float* beta,
                            const void* density_feature, const void* semantic,
                            const void* rgb, const void* base, float* bev_rgb,
                            float* bev_seg, float* bev_height, float* voxel_density,
                            float* voxel_output, const float* ozs_host, void* workspace,
                            size_t workspace_bytes, int flags, void* stream);

/*
 * The render forward as ONE launch (ABI 6): volume_rendering_from_multiple_views, bv2:396-467 -- camera branch
 * (bv2:396-440) and BEV branch (bv2:408-418, 442-461) consume the same four volumes in the reference's one function,
 * and here in one grid: the camera branch's 8 x 8 ray tiles are the first workgroups, the BEV branch's column blocks
 * the ones behind them, so the BEV blocks fill the slots the camera tiles' long tail leaves idle (no fork, no event,
 * no second queue).  Same results as vamp_render_camera_forward_ex(VAMP_CAMFWD_DIRECT) + vamp_render_bev_forward_ex
 * bit for bit (the same device functions).  Early ray termination is on (the data-independent forward keeps its two
 * launches).  Arguments as in those two calls; `workspace` (>= vamp_render_workspace_bytes(d), plus
 * vamp_render_samples_bytes(d) with VAMP_RENDERFWD_SAVE_SAMPLES) receives the termination table and the kept sample
 * rows, `bev_workspace` (vamp_render_bev_workspace_bytes(d), only with VAMP_RENDERFWD_BEV_SAVE) the BEV samples.
 * vamp_render_forward_merged_supported: 1 when the shapes qualify (at most 128 samples per ray, the one-kernel BEV
 * forward's limits) AND ozs_host fits the BEV slabs (see vamp_render_bev_forward_ex); the call itself returns
 * VAMP_EINVAL otherwise -- the caller then issues the two calls.
 * grad_beta_zero (may be NULL): one float the launch sets to zero -- the accumulator a training caller will hand to
 * vamp_render_bev_backward* / vamp_render_camera_backward* as grad_beta, which ADD to it: a one-element fill launch
 * at the head of the backward costs a replayed step ~10 us.
 */
#define VAMP_RENDERFWD_SAVE_SAMPLES 1   /* = VAMP_CAMFWD_SAVE_SAMPLES */
#define VAMP_RENDERFWD_BEV_SAVE 2       /* = VAMP_BEVFWD_SAVE */
/* training: the camera tiles also do the RANK PASS of the camera backward's cell sort -- every kept inside sample is
   counted into its cell and takes its rank there, behind its channel loads.  The caller finishes the prepare step with
   vamp_render_camera_prepare_ex(.., VAMP_CAMPREP_RANKED, stream) (the cell scan: one small kernel, on any
   stream ordered behind this call); afterwards `workspace` holds what vamp_render_camera_prepare_ex
   (VAMP_CAMPREP_TERM_VALID) leaves, and the backward takes VAMP_CAMBWD_CELLS_VALID.  The three launches on two streams
   of a training forward (camera kernel, BEV forward, prepare pass beside it) become one launch + one small one.
   COUNTERS_CLEAN: as VAMP_CAMPREP_COUNTERS_CLEAN, a promise about the counter region of this descriptor in this
   buffer (otherwise the counters are zero-filled first). */
#define VAMP_RENDERFWD_RANK 4
#define VAMP_RENDERFWD_COUNTERS_CLEAN 8
int vamp_render_forward_merged_supported(const VampRenderDesc* d, const float* ozs_host);
int vamp_render_forward_merged(const VampRenderDesc* d, const float* mats, const float* us, const float* vs,
                               const float* ds, const float* mids, const float* oxs, const float* oys,
                               const float* ozs, const float* ozs_host, const float* bev_mids, const float* beta,
                               const void* density_feature, const void* semantic, const void* rgb,
                               const void* base, float* rgb_out, float* seg_out, float* depth_out,
                               float* bev_rgb, float* bev_seg, float* bev_height, float* voxel_density,
                               float* voxel_output, void* workspace, size_t workspace_bytes,
                               void* bev_workspace, size_t bev_workspace_bytes, float* grad_beta_zero, int flags,
                               void* stream);

/*
 * BEV branch, backward.  The four volume gradients are ACCUMULATED into (so that
 * the camera-branch backward can run first into the same buffers); grad_base is
 * written only by this call and must be zero-filled (or hold a running sum).
 * ozs_host is a HOST copy of ozs (used to find the volume planes the det grid
 * touches); workspace needs vamp_render_bev_workspace_bytes(d) bytes.  With
 * ozs_host == NULL the call takes the slower float-atomic formulation (which the
 * tests use as the independent cross-check of the gather).
 */
size_t vamp_render_bev_workspace_bytes(const VampRenderDesc* d);
int vamp_render_bev_backward(const VampRenderDesc* d, const float* oxs, const float* oys,
                             const float* ozs, const float* bev_mids, const float* beta,
                             const void* density_feature, const void* semantic,
                             const void* rgb, const void* base, const float* g_bev_rgb,
                             const float* g_bev_seg, const float* g_bev_height,
                             const float* g_voxel_density, const float* g_voxel_output,
                             float* grad_density_feature, float* grad_semantic,
                             float* grad_rgb, float* grad_base, float* grad_beta,
                             const float* ozs_host, void* workspace, size_t workspace_bytes,
                             void* stream);

/*
 * The same with flags: an OVERWRITE bit makes the call write the named gradients instead of
 * adding to them (voxel planes the det grid does not touch get zeros), which saves the zero fill
 * and the read-modify-write; run it BEFORE vamp_render_camera_backward_acc(..ACCUMULATE) then.
 */
#define VAMP_BEVBWD_OVERWRITE_BASE 1   /* grad_base */
#define VAMP_BEVBWD_OVERWRITE_CAM 2    /* grad_density_feature, grad_semantic, grad_rgb */
#define VAMP_BEVBWD_SKIP_BASE 16        /* first half of a split pair: q, scan, the composited channels' gather (what the camera gather waits for) ... */
#define VAMP_BEVBWD_ONLY_BASE 8         /* ... second half: the beta reduction and the pass-through (grad_base) gather, which nobody waits for; give both calls the same OVERWRITE flags, and issue both */
#define VAMP_BEVBWD_TABLE_VALID 32      /* the workspace still holds the axis tables of an earlier call with the same grids (both halves write their own) */
#define VAMP_BEVBWD_SAVED_VALID 4      /* the workspace holds what vamp_render_bev_forward_ex(.., VAMP_BEVFWD_SAVE) kept */
int vamp_render_bev_backward_ex(const VampRenderDesc* d, const float* oxs, const float* oys,
                             const float* ozs, const float* bev_mids, const float* beta,
                             const void* density_feature, const void* semantic,
                             const void* rgb, const void* base, const float* g_bev_rgb,
                             const float* g_bev_seg, const float* g_bev_height,
                             const float* g_voxel_density, const float* g_voxel_output,
                             float* grad_density_feature, float* grad_semantic,
                             float* grad_rgb, float* grad_base, float* grad_beta,
                             const float* ozs_host, void* workspace, size_t workspace_bytes,
                             int flags, void* stream);

/*
 * What vamp_render_bev_backward_ex(d, .., ozs_host, .., flags, ..) will launch (ABI 10): every choice the call makes
 * from the descriptor, the host heights and the flags, as numbers.  A pure host function -- no HIP call, no GPU --
 * and the very function the backward asks before it launches.  Returns VAMP_OK, or the code (and vamp_last_error
 * message) with which the backward refuses the same arguments: more than 64 heights, ONLY_BASE with SKIP_BASE,
 * tensors beyond the column gather's 32-bit offsets.  Fields a path does not use are 0.
 * The one input the plan does not see is whether g_voxel_output is NULL: seg_gather, base_body and beta_reduce say
 * what a call WITH g_voxel_output does; without it the seg_gather launch is dropped and base_body / beta_reduce
 * take the *_no_vo values.
 */
enum { VAMP_BEVPLAN_PATH_V1 = 0,      /* ozs_host == NULL: the float-atomic splat (zero_* fills in front of it) */
       VAMP_BEVPLAN_PATH_NOOP = 1,    /* ozs_host == NULL with ONLY_BASE: the SKIP_BASE call of the pair did it all */
       VAMP_BEVPLAN_PATH_CELL = 2 };  /* scan + gathers */
enum { VAMP_BEVPLAN_SCAN_NONE = 0, VAMP_BEVPLAN_SCAN_QSCAN21 = 1,   /* bev_qscan_saved_kernel<21> */
       VAMP_BEVPLAN_SCAN_QSCAN0 = 2,                                /* bev_qscan_saved_kernel<0> */
       VAMP_BEVPLAN_SCAN_Q_SCAN = 3 };                              /* bev_q_kernel, then bev_scan_kernel */
enum { VAMP_BEVPLAN_BODY_NONE = 0, VAMP_BEVPLAN_BODY_COMP = 1,      /* bev_gather_comp_kernel */
       VAMP_BEVPLAN_BODY_PASS = 2,                                  /* bev_gather_pass_kernel */
       VAMP_BEVPLAN_BODY_COL = 3,                                   /* bev_gather_col_kernel */
       VAMP_BEVPLAN_BODY_ZERO = 4 };                                /* a zero fill of grad_base */
enum { VAMP_BEVPLAN_BETA_NONE = 0,
       VAMP_BEVPLAN_BETA_TAIL_COMP = 1,   /* first workgroup of the composited gather (comp_body) */
       VAMP_BEVPLAN_BETA_TAIL_BASE = 2,   /* first workgroup of the base gather (base_body PASS or COL) */
       VAMP_BEVPLAN_BETA_LAUNCH = 3,      /* a launch of its own behind the gathers */
       VAMP_BEVPLAN_BETA_EARLY = 4 };     /* outside: a launch of its own right behind the scan */
typedef struct VampBevBackwardPlan {
  int64_t scan_lds;            /* dynamic LDS bytes of the scan body (Q_SCAN: of bev_q_kernel; bev_scan_kernel has none) */
  int32_t path;                /* VAMP_BEVPLAN_PATH_* */
  int32_t z_lo, z_hi;          /* volume planes the lattice touches, clamped to the volume */
  int32_t outside;             /* z_lo > z_hi: only zeros (and, sdf density, d beta) to write */
  int32_t zero_cam, zero_base; /* zero fills in front of a body that adds (v1 splat, generic gather) or of nothing (outside):
                                  grad_density_feature / grad_semantic / grad_rgb, and grad_base where it is not NULL */
  int32_t scan;                /* VAMP_BEVPLAN_SCAN_* */
  int32_t scan_grid[3];        /* grid of bev_qscan_saved_kernel, or of bev_scan_kernel */
  int32_t q_grid[3];           /* grid of bev_q_kernel (Q_SCAN) */
  int32_t scan_waves;          /* waves per workgroup of the scan body */
  int32_t raise_lds;           /* the dynamic-LDS limit is raised first (bev_q_kernel above 60 KB) */
  int32_t beta_parts;          /* d beta partial sums the scan leaves, and the reduction adds up */
  int32_t fits;                /* the column gathers apply (else the generic gather) */
  int32_t nseg, zseg;          /* z segments of the column gather, and planes per segment */
  int32_t comp_ok, pass_ok;    /* tensors within the byte offsets of the composited / pass-through body */
  int32_t build_table;         /* bev_axis_table_kernel runs (fits, no TABLE_VALID) */
  int32_t table;               /* which of the workspace's two axis tables: 1 for ONLY_BASE */
  int32_t comp_body;           /* semantic + rgb + density: NONE, COMP or COL */
  int32_t comp_overwrite;      /* its <.., true> variant (OVERWRITE_CAM) */
  int32_t seg_gather;          /* the cat_seg column launch of voxel_output's semantic part */
  int32_t base_body;           /* grad_base: NONE, PASS, COL or ZERO */
  int32_t base_overwrite;      /* its <.., true> variant (OVERWRITE_BASE) */
  int32_t base_body_no_vo;     /* g_voxel_output == NULL: NONE or ZERO */
  int32_t generic;             /* bev_gather_generic_kernel over planes z_lo .. z_hi, behind the zero_* fills */
  int32_t beta_reduce;         /* VAMP_BEVPLAN_BETA_* */
  int32_t beta_reduce_no_vo;   /* g_voxel_output == NULL */
  int32_t reserved[6];         /* 0 */
} VampBevBackwardPlan;
int vamp_render_bev_backward_plan(const VampRenderDesc* d, const float* ozs_host, int flags, VampBevBackwardPlan* out);

/*
 * Diagnostics: inside-mask (bv2:405-407) and floor taps of the camera branch's
 * trilinear sample per (b, n, d < D-1, h, w); geometry as in the forward.
 */
int vamp_render_indices(const VampRenderDesc* d, const float* geom, const float* mats,
                        const float* us, const float* vs, const float* ds, uint8_t* inside,
                        int16_t* ix0, int16_t* iy0, int16_t* iz0, void* stream);

/*
 * The same diagnostic for the one-kernel camera forward (render_cam_direct.hip): inside mask and floor
 * taps of every sample [B, N, D-1, fH, fW] as THAT kernel evaluates them (its sample coordinates come
 * from an fp64 line per ray with a wave-level fallback to the fp32 chain of bv2:328-349 next to the
 * faces of the volume); fxyz (may be NULL) [B, N, D-1, fH, fW, 3] receives the continuous tap
 * coordinates.  The mask is the reference's bit for bit; a floor tap can differ from the reference's
 * where a coordinate lies within ~1e-5 of an integer (the trilinear sample is continuous there).
 */
int vamp_render_camera_direct_taps(const VampRenderDesc* d, const float* mats, const float* us,
                                   const float* vs, const float* ds, uint8_t* inside, int16_t* ix0,
                                   int16_t* iy0, int16_t* iz0, float* fxyz, void* stream);

/* get_geometry (bv2:314-349) + nan_to_num(-1e3) (bv2:612): geom [B,N,D,fH,fW,3]. */
int vamp_frustum_geometry(const VampRenderDesc* d, const float* mats, const float* us,
                          const float* vs, const float* ds, float* geom, void* stream);

/* --------------------------------------------------------------------------
 * Point resampling: the occupancy and lidar-point queries of
 * base_vampire2.py:576-609 -- F.grid_sample(volume, points, align_corners=True) with the
 * points normalised by the seg bounds.
 *   occ_logits  bv2:603   padding BORDER                     (points = bda-rotated occ grid, bv2:599-602)
 *   occ_density bv2:604   padding ZEROS, activation = 1      (density(density_feature) is sampled)
 *   pts_logits  bv2:590   padding BORDER, channel_last_out   (lidar points of one sample, B = 1)
 *   pts_sdf     bv2:594   padding ZEROS, mask_outside = 1
 * -------------------------------------------------------------------------- */
#define VAMP_PAD_ZEROS 0
#define VAMP_PAD_BORDER 1
typedef struct {
  int32_t B, C;            /* samples, channels of the volume (C <= 32; C == 1 with activation) */
  int32_t Z, Y, X;
  float lo[3], span[3];    /* (p - lo) / span * 2 - 1 is the normalised coordinate (bv2:581-586) */
  int32_t padding;         /* VAMP_PAD_ZEROS | VAMP_PAD_BORDER */
  int32_t mask_outside;    /* multiply by all(-1 <= n <= 1) (bv2:587-589, 595) */
  int32_t activation;      /* sample density(volume) instead of volume (bv2:604) */
  int32_t density_mode;    /* VAMP_DENSITY_*; with sdf_bias / beta_min as in VampRenderDesc */
  float sdf_bias, beta_min;
  int32_t channel_last_out;/* out / grad_out are [B, P, C] instead of [B, C, P] */
  int32_t in_dtype;        /* dtype of `volume` */
  int32_t lattice[3];      /* optional hint: the P points are a row-major n0 x n1 x n2 lattice (n2
                              fastest) whose axis 0 runs along the volume's x, as the occ grid does
                              ([200, 200, 16, 3], bv2:295-312): threads then walk axis 0 so that
                              neighbouring lanes read neighbouring voxels.  0, 0, 0 = no structure */
} VampSampleDesc;

/*
 * volume [B, C, Z, Y, X]; points [B, P, 3] fp32 ego-frame (x, y, z), P = points_per_sample;
 * out [B, C, P] (or [B, P, C]) fp32; beta as in the render entry points (read only with
 * activation and the sdf density).
 */
int vamp_sample_points_forward(const VampSampleDesc* d, const void* volume, const float* beta,
                               const float* points, int64_t points_per_sample, float* out,
                               void* stream);
size_t vamp_sample_points_workspace_bytes(const VampSampleDesc* d, int64_t points_per_sample);
/* grad_volume [B, C, Z, Y, X] fp32 is fully overwritten; grad_beta (1 float) is ACCUMULATED into. */
int vamp_sample_points_backward(const VampSampleDesc* d, const void* volume, const float* beta,
                                const float* points, int64_t points_per_sample,
                                const float* grad_out, float* grad_volume, float* grad_beta,
                                void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * The four point queries of a step in one call (base_vampire2.py:576-609): the same values as the
 * four vamp_sample_points_forward calls above -- the same fp32 chain, bit for bit -- from packed
 * points with per-sample counts, and ONE backward: one cell list over both point sets and all
 * samples, one gather that overwrites grad_semantic and grad_density once each.
 *   pts_logits  [B, M, K]       bv2:590   border padding, channel-last   (lidar points)
 *   pts_sdf     [B, M]          bv2:594-595  zeros padding x inside mask (when want_sdf)
 *   occ_logits  [B, K, P_occ]   bv2:603   border padding                 (the bda-rotated occ grid, bv2:599-602)
 *   occ_density [B, 1, P_occ]   bv2:604   zeros padding of density(density_feature); no tanh (bv2:609)
 * counts [B] int32 on the device (NULL: all M rows), clamped to [0, M] in the kernels: rows i >= counts[b] of
 * `points` and of the upstream gradients are never read, their output rows are exact 0.
 * Launches do not depend on B; no float atomics on the volumes' gradients; no host synchronisation.
 * -------------------------------------------------------------------------- */
typedef struct {
  int32_t B, K;            /* samples, semantic channels (K + 1 <= 32: the backward's widest gradient row) */
  int32_t Z, Y, X;
  float lo[3], span[3];    /* as in VampSampleDesc (bv2:581-586) */
  int32_t density_mode;    /* VAMP_DENSITY_*; with sdf_bias / beta_min as in VampRenderDesc */
  float sdf_bias, beta_min;
  int32_t sem_dtype, den_dtype;   /* VAMP_F32 | VAMP_BF16 of `semantic` and of `density` */
  int32_t M;               /* lidar-point capacity per sample; 0 = no lidar part */
  int32_t want_sdf;        /* pts_sdf is asked for (the sdf density, bv2:593) */
  int32_t P_occ;           /* occupancy points per sample; 0 = no occupancy part */
  int32_t occ_shared;      /* occ_points is [1, P_occ, 3] for all samples (the static grid of
                              base_lss_impaintor.py:611-616) instead of [B, P_occ, 3] */
  int32_t lattice[3];      /* the occupancy points' lattice hint, as in VampSampleDesc */
} VampQueryDesc;

/* 1 when the entry points below take the descriptor (bv2:576-609 at these shapes), else 0 */
int vamp_point_queries_supported(const VampQueryDesc* d);
/* bytes of the backward's workspace (bv2:576-609); 0 for a descriptor that is refused */
size_t vamp_point_queries_workspace_bytes(const VampQueryDesc* d);
/*
 * bv2:590, 594-595, 603, 604.  semantic [B, K, Z, Y, X], density [B, 1, Z, Y, X] (may be NULL when neither
 * want_sdf nor P_occ asks for it); points [B, M, 3] fp32 ego-frame; occ_points [B | 1, P_occ, 3]; beta as in the
 * render entry points (read only for occ_density with the sdf density).  Outputs fp32, fully overwritten.
 */
int vamp_point_queries_forward(const VampQueryDesc* d, const void* semantic, const void* density,
                               const float* beta, const float* points, const int32_t* counts,
                               const float* occ_points, float* pts_logits, float* pts_sdf,
                               float* occ_logits, float* occ_density, void* stream);
/*
 * The backward of bv2:590, 594-595, 603, 604 in one pass.  g_* are the upstream gradients of the four outputs
 * (any may be NULL: zero).  grad_semantic [B, K, Z, Y, X] and grad_density [B, 1, Z, Y, X] (NULL where
 * `density` may be) fp32 are fully overwritten, once; grad_beta (1 float, may be NULL) is ACCUMULATED into.
 */
int vamp_point_queries_backward(const VampQueryDesc* d, const void* density, const float* beta,
                                const float* points, const int32_t* counts, const float* occ_points,
                                const float* g_pts_logits, const float* g_pts_sdf,
                                const float* g_occ_logits, const float* g_occ_density,
                                float* grad_semantic, float* grad_density, float* grad_beta,
                                void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Producer / consumer steps either side of the path.
 *   depth softmax  base_vampire2.py:550  `mapping_along_depth(src).softmax(dim=1)`:
 *                  logits [images, D, HW] (fp32 | bf16, images = B * N cameras, HW = fH * fW)
 *                  -> depth [images, D, HW] fp32, the `depth` argument of vamp_lift_forward.
 *   density gate   base_vampire2.py:627-630  `voxel_output * bev_density.tanh()` (sdf density) or
 *                  `voxel_output * bev_density` (naive): voxel_output [B, C, cells], voxel_density
 *                  [B, 1, cells] (cells = oZ * oY * oX, both outputs of vamp_render_forward) ->
 *                  out [B, C, cells], the input of the `voxel_output` 1x1 conv.
 * All tensors contiguous; nothing is retained.
 * -------------------------------------------------------------------------- */
int vamp_depth_softmax_forward(int64_t images, int32_t D, int64_t HW, const void* logits,
                               int32_t in_dtype, float* depth, void* stream);
/* grad_logits = depth * (grad_depth - sum_d depth * grad_depth), fully overwritten */
int vamp_depth_softmax_backward(int64_t images, int32_t D, int64_t HW, const float* depth,
                                const float* grad_depth, float* grad_logits, void* stream);
int vamp_density_gate_forward(int64_t B, int32_t C, int64_t cells, int32_t density_mode,
                              const float* voxel_output, const float* voxel_density, float* out,
                              void* stream);
/* grad_voxel_output [B, C, cells] and grad_voxel_density [B, 1, cells] are fully overwritten */
int vamp_density_gate_backward(int64_t B, int32_t C, int64_t cells, int32_t density_mode,
                               const float* grad_out, const float* voxel_output,
                               const float* voxel_density, float* grad_voxel_output,
                               float* grad_voxel_density, void* stream);

/*
 * Consumer fusion (base_vampire2.py:627-632 with the conv of :203-209): the density gate and
 * the `voxel_output` 1x1 convolution in one kernel each way, on the fp32 matrix cores --
 *   out[b, o, cell] = bias[o] + sum_ci weight[o, ci] * voxel_output[b, ci, cell] * gate(voxel_density[b, ci % oZ, cell])
 * with ci = c * oZ + z (the reference's reshape(B, C * oZ, oY, oX)), cell = oY * oX positions of the BEV
 * plane, gate = tanh (sdf density) or identity (naive).  voxel_output [B, C, oZ, cells], voxel_density
 * [B, 1, oZ, cells] (outputs of vamp_render_forward), weight [Cout, C * oZ] (= Conv2d.weight), bias [Cout] or
 * NULL, out [B, Cout, cells]; fp32, contiguous.  The gated tensor is never materialised.
 * Shapes: C * oZ <= 160, Cout <= 80, oZ <= 32, and the backward's LDS image must fit the CU's 160 KB, which caps
 * oZ at 20 when C * oZ > 64 and Cout > 16 (vamp_gate_conv1x1_supported; else callers keep aten).
 */
int vamp_gate_conv1x1_supported(int32_t C, int32_t oZ, int32_t Cout);
size_t vamp_gate_conv1x1_workspace_bytes(int32_t C, int32_t oZ, int32_t Cout);
int vamp_gate_conv1x1_forward(int64_t B, int32_t C, int32_t oZ, int64_t cells, int32_t Cout,
                              int32_t density_mode, const float* voxel_output,
                              const float* voxel_density, const float* weight, const float* bias,
                              float* out, void* stream);
/* grad_voxel_output [B, C, oZ, cells], grad_voxel_density [B, 1, oZ, cells], grad_weight [Cout, C * oZ] and
 * grad_bias [Cout] (may be NULL) are fully overwritten; deterministic (no float atomics). */
int vamp_gate_conv1x1_backward(int64_t B, int32_t C, int32_t oZ, int64_t cells, int32_t Cout,
                               int32_t density_mode, const float* grad_out, const float* voxel_output,
                               const float* voxel_density, const float* weight,
                               float* grad_voxel_output, float* grad_voxel_density, float* grad_weight,
                               float* grad_bias, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * BEVDepth-style voxel pooling (north_star's "LSS frustum-to-voxel pooling op").
 * NOT in /root/reference at the pinned commit (its backbones lift with grid_sample = vamp_lift_*); this
 * follows the published BEVDepth operator `voxel_pooling(geom_xyz, input_features, voxel_num)`:
 *   out[b, y, x, :] = sum of feat[b, p, :] over the points p with 0 <= geom[b, p] = (x, y, z) < (nx, ny, nz).
 * geom_xyz [B, P, 3] int32 voxel indices (P = N * D * H * W frustum points), feat [B, P, C] (in_dtype),
 * out [B, ny, nx, C] fp32, fully overwritten (the caller permutes to [B, C, ny, nx] as upstream does).
 * Sort-then-own instead of upstream's float atomics; sums run in list order (last-bit run-to-run
 * variation, like upstream).  Parity unpinned: checked against a numpy scatter-add of the definition.
 * -------------------------------------------------------------------------- */
typedef struct VampPoolDesc {
  int32_t B, C;          /* samples, channels                                   */
  int64_t P;             /* frustum points per sample                           */
  int32_t nx, ny, nz;    /* voxel_num                                           */
  int32_t in_dtype;      /* VAMP_F32 | VAMP_BF16 for feat                       */
} VampPoolDesc;
size_t vamp_voxel_pooling_workspace_bytes(const VampPoolDesc* d);
int vamp_voxel_pooling_forward(const VampPoolDesc* d, const int32_t* geom_xyz, const void* feat, float* out,
                               void* workspace, size_t workspace_bytes, void* stream);
/* grad_feat [B, P, C] fp32 is fully overwritten: the row of the point's cell, zeros outside the grid */
int vamp_voxel_pooling_backward(const VampPoolDesc* d, const int32_t* geom_xyz, const float* grad_out,
                                float* grad_feat, void* stream);

/* --------------------------------------------------------------------------
 * Trilinear resize inside the 3-D UNet between lift and render (first piece):
 * F.interpolate(x, size, mode='trilinear', align_corners=True), base_vampire2.py:66, 72.
 * in [planes, iz, iy, ix] -> out [planes, oz, oy, ox], planes = batch * channels, fp32 contiguous.
 * The backward is a gather over a small per-axis table built in `workspace` (no float atomics);
 * it supports resize factors up to about 6 per axis and returns VAMP_EINVAL beyond.
 * -------------------------------------------------------------------------- */
int vamp_upsample_trilinear_forward(int64_t planes, int32_t iz, int32_t iy, int32_t ix, int32_t oz,
                                    int32_t oy, int32_t ox, const float* in, float* out,
                                    void* stream);
size_t vamp_upsample_trilinear_workspace_bytes(int32_t iz, int32_t iy, int32_t ix);
/* the same with 16-bit tensors (a mixed-precision UNet): dtype = VAMP_F32 | VAMP_BF16 | VAMP_F16 for in / out
   (and grad_out / grad_in below); fp32 arithmetic */
int vamp_upsample_trilinear_forward_ex(int64_t planes, int32_t iz, int32_t iy, int32_t ix, int32_t oz,
                                       int32_t oy, int32_t ox, int32_t dtype, const void* in, void* out,
                                       void* stream);
int vamp_upsample_trilinear_backward_ex(int64_t planes, int32_t iz, int32_t iy, int32_t ix, int32_t oz,
                                        int32_t oy, int32_t ox, int32_t dtype, const void* grad_out, void* grad_in,
                                        void* workspace, size_t workspace_bytes, void* stream);
/* 1 when the backward's gather table covers this scale (about out / in <= 6 per axis), else 0:
 * callers fall back to F.interpolate then */
int vamp_upsample_trilinear_supported(int32_t iz, int32_t iy, int32_t ix, int32_t oz, int32_t oy, int32_t ox);
/* grad_in [planes, iz, iy, ix] is fully overwritten */
int vamp_upsample_trilinear_backward(int64_t planes, int32_t iz, int32_t iy, int32_t ix, int32_t oz,
                                     int32_t oy, int32_t ox, const float* grad_out, float* grad_in,
                                     void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * 2-D bilinear resize of the rendered maps between render and losses:
 * F.interpolate(x, size, mode='bilinear', align_corners=True) -- the x4 `upsample2d` of the rgb, seg-logit and depth
 * camera maps, base_vampire2.py:616-626, and the 0.5x resize behind `voxel_output` on a 256-cell grid,
 * base_vampire2.py:203-209.  in [planes, ih, iw] -> out [planes, oh, ow], planes = batch * channels, fp32 contiguous.
 * One call takes up to VAMP_RESIZE2D_MAX_SEGS tensors (segments) that share the four sizes: one kernel launch on
 * `stream` each way, the pointers travel inside the launch arguments (capturable in a graph).  The backward is a
 * separable gather in a fixed order (no float atomics, bitwise repeatable) that overwrites every element of every
 * segment's `dst`, untouched source pixels with 0.
 * -------------------------------------------------------------------------- */
#define VAMP_RESIZE2D_MAX_SEGS 4
#define VAMP_RESIZE2D_PLANE_GROUP 8   /* planes one forward thread walks with its taps                            */
#define VAMP_RESIZE2D_BAND_ROWS 8     /* source rows one backward workgroup owns                                  */
#define VAMP_RESIZE2D_COL_CHUNK 256   /* source columns one backward workgroup owns                               */
#define VAMP_RESIZE2D_STRIP_CHUNK 256 /* gradient columns one 16-byte load of a wave covers                       */
#define VAMP_RESIZE2D_STRIP_MAX 1088  /* gradient columns (rounded out to multiples of 4) a column chunk may span */
#define VAMP_RESIZE2D_MAX_RUN 16      /* outputs along x whose taps include one source column                     */
typedef struct VampResize2dSeg {
  const void* src;       /* forward: in [planes, ih, iw]; backward: grad_out [planes, oh, ow]   */
  void* dst;             /* forward: out [planes, oh, ow]; backward: grad_in [planes, ih, iw]   */
  int64_t planes;        /* 0 < planes < 65536                                                   */
} VampResize2dSeg;
typedef struct VampResize2dDesc {
  int32_t ih, iw, oh, ow;
  int32_t nseg;          /* 1 .. VAMP_RESIZE2D_MAX_SEGS                                          */
  int32_t reserved;
  VampResize2dSeg seg[VAMP_RESIZE2D_MAX_SEGS];
} VampResize2dDesc;
/* 1 when both entry points take these sizes, else 0 (callers fall back to F.interpolate then): any ratio along y;
 * along x the run of outputs per source column must fit VAMP_RESIZE2D_MAX_RUN and the outputs of a column chunk
 * VAMP_RESIZE2D_STRIP_MAX -- every out / in <= 4.1, the identity and every downsampling pass */
int vamp_resize2d_supported(int32_t ih, int32_t iw, int32_t oh, int32_t ow);
/* scratch the backward needs: 0 in this version (its run tables live in registers and LDS); NULL is accepted then */
size_t vamp_resize2d_workspace_bytes(int32_t ih, int32_t iw, int32_t oh, int32_t ow);
int vamp_resize2d_forward(const VampResize2dDesc* d, void* stream);
int vamp_resize2d_backward(const VampResize2dDesc* d, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * 3x3x3 / stride 1 / padding 1 / no-bias Conv3d of the UNet between lift and render (SURVEY 8f
 * N3): nn.Conv3d(cin, cout, 3, 1, 1, bias=False) with cin, cout in {16, 32} -- init_dres, conv2,
 * conv4, conv5, conv6 of the two Hourglass3D blocks, base_vampire2.py:20, 40-60.  fp32 NCDHW
 * tensors, weight [cout, cin, 3, 3, 3]; fp32 matrix cores (exact fp32 products).
 * -------------------------------------------------------------------------- */
typedef struct {
  int32_t B, cin, cout, Z, Y, X;
} VampConvDesc;
/* 1 when the three entry points below accept the descriptor (cin, cout in {16, 32};
   (cin + cout) * X <= 12288 and the LDS row images of the weight gradient fit), else 0 */
int vamp_conv3d_supported(const VampConvDesc* d);
int vamp_conv3d_forward(const VampConvDesc* d, const float* in, const float* weight, float* out,
                        void* stream);
int vamp_conv3d_backward_data(const VampConvDesc* d, const float* grad_out, const float* weight,
                              float* grad_in, void* stream);
size_t vamp_conv3d_workspace_bytes(const VampConvDesc* d);
/* grad_weight [cout, cin, 3, 3, 3] is fully overwritten; workspace holds the per-workgroup partial
   sums (vamp_conv3d_workspace_bytes) */
int vamp_conv3d_backward_weight(const VampConvDesc* d, const float* in, const float* grad_out,
                                float* grad_weight, void* workspace, size_t workspace_bytes,
                                void* stream);

/*
 * The same layers under the reference's `precision=16` (base_cli.py:77; autocast hands the layers of
 * base_vampire2.py:20, 40-60 bf16 activations and weights): bf16 NCDHW in, fp32 accumulate on the bf16
 * matrix cores (v_mfma_f32_16x16x32_bf16), bf16 NCDHW out; weight [cout, cin, 3, 3, 3] bf16; 1 <= cin, cout
 * <= 32, X % 4 == 0 (vamp_conv3d_bf16_supported).  grad_weight is fp32 [cout, cin, 3, 3, 3].
 */
int vamp_conv3d_bf16_supported(const VampConvDesc* d);
int vamp_conv3d_bf16_forward(const VampConvDesc* d, const void* in, const void* weight, void* out, void* stream);
int vamp_conv3d_bf16_backward_data(const VampConvDesc* d, const void* grad_out, const void* weight, void* grad_in,
                                   void* stream);
size_t vamp_conv3d_bf16_workspace_bytes(const VampConvDesc* d);
int vamp_conv3d_bf16_backward_weight(const VampConvDesc* d, const void* in, const void* grad_out, float* grad_weight,
                                     void* workspace, size_t workspace_bytes, void* stream);
/* the same three with the 16-bit type as an argument: dtype = VAMP_BF16 or VAMP_F16 (IEEE half, what Lightning's
   `precision=16` autocasts to: v_mfma_f32_16x16x32_f16); shapes / workspace as the bf16 entry points */
int vamp_conv3d_half_forward(const VampConvDesc* d, int32_t dtype, const void* in, const void* weight, void* out,
                             void* stream);
int vamp_conv3d_half_backward_data(const VampConvDesc* d, int32_t dtype, const void* grad_out, const void* weight,
                                   void* grad_in, void* stream);
int vamp_conv3d_half_backward_weight(const VampConvDesc* d, int32_t dtype, const void* in, const void* grad_out,
                                     float* grad_weight, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The stride-2 layers of the same UNet under a 16-bit autocast: nn.Conv3d(cin, cout, 3, stride=2, padding=1,
 * bias=False) -- Hourglass3D.conv1 and conv3, base_vampire2.py:34-46.  Here the descriptor holds the INPUT tensor
 * [B, cin, Z, Y, X]; the output is [B, cout, Zo, Yo, Xo] with Zo = (Z - 1) / 2 + 1, Yo = (Y - 1) / 2 + 1,
 * Xo = (X - 1) / 2 + 1 (odd Z and Y are fine).  16-bit NCDHW in and out (dtype = VAMP_BF16 or VAMP_F16), fp32
 * accumulation on v_mfma_f32_16x16x32_{bf16,f16}; weight [cout, cin, 3, 3, 3] of the same 16-bit type.  One shape rule
 * for the three launches (vamp_conv3d_half_s2_supported): 1 <= cin, cout <= 32, B, Z, Y > 0, X >= 8, X % 4 == 0 and
 * Z * Y * X * 64 < 2^31.  grad_in [B, cin, Z, Y, X] is fully overwritten (every element once, no atomics);
 * grad_weight is fp32 [cout, cin, 3, 3, 3], fully overwritten and bitwise repeatable; the workspace
 * (vamp_conv3d_half_s2_workspace_bytes) holds the per-workgroup partial sums.
 */
int vamp_conv3d_half_s2_supported(const VampConvDesc* d);
size_t vamp_conv3d_half_s2_workspace_bytes(const VampConvDesc* d);
int vamp_conv3d_half_s2_forward(const VampConvDesc* d, int32_t dtype, const void* in, const void* weight, void* out,
                                void* stream);
int vamp_conv3d_half_s2_backward_data(const VampConvDesc* d, int32_t dtype, const void* grad_out, const void* weight,
                                      void* grad_in, void* stream);
int vamp_conv3d_half_s2_backward_weight(const VampConvDesc* d, int32_t dtype, const void* in, const void* grad_out,
                                        float* grad_weight, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same convolutions with an epilogue at the point where they store their accumulators:
 *     y = act(conv(x, w) + bias + residual)
 * in 1 .. VAMP_CONV_EPI_MAX_SEGS segments of output channels.  A segment is a channel range [c0, c0 + nch), an
 * optional fp32 bias[nch], an optional residual, an activation and an output tensor of its own, contiguous
 * [B, nch, Zo, Yo, Xo] (the convolution's output volume); the residual has the output's shape and type.  The output
 * type is the kind's compute type (fp32, or `dtype` for the 16-bit kinds), or fp32 from a 16-bit kind when out_f32
 * is 1; the segments of one call share out_f32.  An ordinary layer is one segment over all of cout; the three heads (density / logits / rgb + sigmoid) are
 * three segments of one convolution written straight into three tensors.  Channels that no segment holds are computed
 * and not stored.  The arithmetic order is fixed, fp32, one rounding per step and no contraction: acc + bias, then
 * + residual, then the activation; the result is rounded once to the output type.  leaky_relu is
 * v > 0 ? v : v * slope, sigmoid 1 / (1 + exp(-v)).
 *
 * The plain entry points above launch kernels without any of this.
 *
 * Backward: vamp_conv3d_epilogue_backward computes g_z = g * act'(y) -- leaky: y > 0 ? 1 : slope, sigmoid:
 * y (1 - y) -- from each segment's gradient `grad_out` and output `out` (both of the segment's output type), gathers
 * the segments into ONE grad_z [B, cout, Zo, Yo, Xo] of the compute type (channels outside every segment: 0), rounded
 * once, and -- for every segment with a grad_bias -- sums g_z over samples and voxels, in the segment's own precision
 * (the rounded g_z of a compute-type segment; the fp32 products of an fp32-output segment of a 16-bit kind, whose copy
 * in grad_z is rounded for the convolution's backward alone): float64 partials per workgroup in `workspace`, added in
 * a fixed order by a finishing launch, rounded once to fp32; no atomics, bitwise repeatable.  grad_z is the residual's
 * gradient, and the operand of the existing backward_data / backward_weight entry points.  A residual's gradient is its
 * segment's channels of grad_z as stored: rounded once to the compute type, and for the fp32 residual of an fp32-output
 * segment of a 16-bit kind those 16-bit values widened, not the fp32 products.  `stride` (1 or 2) and `dtype` name the kind: (1, VAMP_F32), (1, 16-bit), (2, 16-bit).
 *
 * Every entry point refuses, before any launch, with VAMP_EINVAL: a descriptor its kind does not take, a NULL
 * required pointer, nseg outside 1 .. 4, a segment outside [0, cout) or overlapping another, an unknown activation,
 * out_f32 = 1 for the fp32 kind or differing between segments, forward tensors off a 16-byte boundary; with VAMP_ENOSPC a workspace below
 * vamp_conv3d_epilogue_workspace_bytes.  "Forward tensors" are in, weight and every segment's out, residual and bias.
 * vamp_conv3d_epilogue_supported answers the same rules (pointers aside) without a GPU and, being a question, leaves
 * vamp_last_error as it was.
 */
enum { VAMP_ACT_NONE = 0, VAMP_ACT_LEAKY_RELU = 1, VAMP_ACT_SIGMOID = 2 };
#define VAMP_CONV_EPI_MAX_SEGS 4
#define VAMP_CONV_EPI_CHUNK 4096      /* voxels of one (sample, channel) a backward workgroup owns */
typedef struct VampConvEpiSeg {
  const float* bias;      /* forward: fp32 [nch] or NULL                                                       */
  const void* residual;   /* forward: [B, nch, Zo, Yo, Xo] of the output type, or NULL                         */
  void* out;              /* forward: the output (written); backward: the same tensor (read; NULL with ACT_NONE) */
  const void* grad_out;   /* backward: the gradient of `out`, of the output type                               */
  float* grad_bias;       /* backward: fp32 [nch] (written) or NULL                                            */
  int32_t c0, nch;        /* output channels [c0, c0 + nch)                                                    */
  int32_t act;            /* VAMP_ACT_*                                                                        */
  int32_t out_f32;        /* 0: the compute type; 1: fp32 (16-bit kinds only)                                  */
  float slope;            /* VAMP_ACT_LEAKY_RELU's negative slope                                              */
  int32_t reserved;
} VampConvEpiSeg;
typedef struct VampConvEpilogue {
  int32_t nseg;           /* 1 .. VAMP_CONV_EPI_MAX_SEGS */
  int32_t reserved;
  VampConvEpiSeg seg[VAMP_CONV_EPI_MAX_SEGS];
} VampConvEpilogue;
int vamp_conv3d_epilogue_supported(const VampConvDesc* d, int32_t stride, int32_t dtype, const VampConvEpilogue* epi);
int vamp_conv3d_epilogue_forward(const VampConvDesc* d, const VampConvEpilogue* epi, const float* in,
                                 const float* weight, void* stream);
int vamp_conv3d_half_epilogue_forward(const VampConvDesc* d, int32_t dtype, const VampConvEpilogue* epi,
                                      const void* in, const void* weight, void* stream);
int vamp_conv3d_half_s2_epilogue_forward(const VampConvDesc* d, int32_t dtype, const VampConvEpilogue* epi,
                                         const void* in, const void* weight, void* stream);
size_t vamp_conv3d_epilogue_workspace_bytes(const VampConvDesc* d, int32_t stride);
int vamp_conv3d_epilogue_backward(const VampConvDesc* d, int32_t stride, int32_t dtype, const VampConvEpilogue* epi,
                                  void* grad_z, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Segmentation metrics (base_exp.py:370-382 training, :634-663 validation, :835-840 submission labels).
 *
 * vamp_confusion_update: for every element i with mask[i] != 0 (mask may be NULL) and, when use_ignore,
 * target[i] != ignore_index, the prediction p = lo + argmax(logits[i, lo:hi]) (torch.argmax: the first
 * maximal index, a NaN above every number and the first NaN wins; bf16 compared after exact conversion to
 * fp32) -- or pred[i] itself for integer predictions -- is counted as
 *     confmat[t, p] += 1   if 0 <= t = target[i] < Kc and 0 <= p < Kc,   else invalid[0] += 1.
 * confmat [Kc, Kc] and invalid [1] are int64 and ACCUMULATED.  Logit layouts, n = B * S elements:
 *   VAMP_SEG_ROWS   logits [n, K], the classes of an element contiguous (point logits);
 *   VAMP_SEG_PLANES logits [B, K, S], element i = b * S + s (the channel-first volume behind the
 *                   backbone's occ_logits.permute(0, 2, 3, 4, 1) view: class stride S = X * Y * Z).
 * target [n] (target_dtype), mask [n] (bool bytes).  Integer predictions: pred [n], layout ROWS, K = 1,
 * lo / hi unused.  Per-workgroup LDS histograms stored to slabs of the workspace
 * (vamp_confusion_workspace_bytes) and added in a fixed order by a second launch: exact, no float atomics,
 * no synchronisation, capturable.  n < 2^31 per call.
 * -------------------------------------------------------------------------- */
enum { VAMP_I64 = 3, VAMP_I32 = 4, VAMP_U8 = 5 };     /* integer tensors of the metric entry points */
enum { VAMP_SEG_ROWS = 0, VAMP_SEG_PLANES = 1 };
typedef struct VampConfDesc {
  int64_t B, S;          /* n = B * S elements (ROWS: B = 1)                                 */
  int32_t K;             /* classes of a logit row (the class dimension); integer predictions: 1 */
  int32_t layout;        /* VAMP_SEG_ROWS | VAMP_SEG_PLANES                                  */
  int32_t pred_dtype;    /* VAMP_F32 | VAMP_BF16 logits, VAMP_I64 | VAMP_I32 predictions       */
  int32_t target_dtype;  /* VAMP_I64 | VAMP_I32 | VAMP_U8                                    */
  int32_t Kc;            /* confusion-matrix classes, 1..32                                   */
  int32_t lo, hi;        /* class window: 0 <= lo < hi <= K and hi - 1 < Kc                   */
  int32_t ignore_index;  /* targets equal to it are skipped when use_ignore = 1               */
  int32_t use_ignore;
  int32_t reserved;      /* 0 */
} VampConfDesc;
size_t vamp_confusion_workspace_bytes(const VampConfDesc* d);
int vamp_confusion_update(const VampConfDesc* d, const void* pred, const void* target, const uint8_t* mask,
                          int64_t* confmat, int64_t* invalid, void* workspace, size_t workspace_bytes,
                          void* stream);
/* vamp_lidarseg_predict: ref_logits[r] = fp32 sum, in increasing point order, of pts_logits[p] (row of K,
 * dtype VAMP_F32 | VAMP_BF16) over the points p with ref_index[p] == r (the reference's zeros + index_add_),
 * labels[r] = lo + argmax(ref_logits[r, lo:hi]) as int64 (a reference point no point maps to has zero logits:
 * label lo).  Points whose index lies outside [0, num_ref) are not summed; their count is written to
 * invalid[0] (int64).  labels [num_ref] and invalid are overwritten.  hi - lo <= 64; P, num_ref < 2^31.
 * Deterministic and bit-exact against a sequential CPU index_add_. */
size_t vamp_lidarseg_workspace_bytes(int64_t P, int64_t num_ref);
int vamp_lidarseg_predict(int64_t P, int32_t K, int32_t dtype, int32_t lo, int32_t hi, const void* pts_logits,
                          const int64_t* ref_index, int64_t num_ref, int64_t* labels, int64_t* invalid,
                          void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Detection post-processing: the reference head's get_bboxes (bev_depth_head.py:381-494, the decode of
 * CenterPointBBoxCoder and the three NMS kinds of :420-475) for all T tasks of a head and all B samples, on the
 * device, with a fixed-capacity output.  Per task t the head tensors are contiguous, all of dtype in_dtype
 * (VAMP_F32 | VAMP_BF16 | VAMP_F16): heatmap [B, ncls[t], H, W], reg [B, 2, H, W], height [B, 1, H, W],
 * dim [B, 3, H, W], rot [B, 2, H, W] (sin, cos), vel [B, 2, H, W] when has_vel.
 *
 *  score      sigmoid as aten computes it: 1 / (1 + expf(-x)) in fp32 (accurate expf), rounded to in_dtype.
 *  candidates the top K = min(max_num, ncls[t] * H * W) of the flattened [ncls, H, W] scores, score descending,
 *             ties by flat index ascending (a NaN ranks above every number).
 *  decode     x = ((W-index + reg0) * out_size_factor) * voxel_size[0] + pc_range[0] (each op rounded, no FMA),
 *             y likewise with the H-index and reg1; z = height; dim = exp(dim) when norm_bbox; rot = atan2(sin,
 *             cos); vel.  Exp and atan2 of 16-bit heads are rounded to in_dtype, as torch computes them.
 *  filter     score > score_threshold (when use_score_threshold; the caller passes the threshold rounded to
 *             in_dtype, as torch compares a tensor with a Python scalar) and, when use_center_range,
 *             post_center_range[0:3] <= (x, y, z) <= post_center_range[3:6].  Survivors keep their order.
 *  NMS        greedy in candidate order per (sample, task), the kept list truncated to post_max_size:
 *               VAMP_NMS_CIRCLE      suppress when dx^2 + dy^2 <= min_radius[t] (circle_nms);
 *               VAMP_NMS_SIZE_AWARE  suppress when |dx| <= (ex_i + ex_j) * thresh_scale[t] / 2 and the same in
 *                                    y, ex = dx |cos yaw| + dy |sin yaw|, ey = dx |sin yaw| + dy |cos yaw|;
 *               VAMP_NMS_ROTATE      candidates truncated to pre_max_size first; suppress when the IoU of the
 *                                    rotated BEV rectangles (x, y, dx, dy, yaw) is > nms_thr[t], IoU =
 *                                    intersection / max(union, 1e-8) (a box with dx or dy <= 0 overlaps nothing).
 *  output     per sample b, the tasks' kept rows in task order: boxes [B, T * P, 9 | 7] fp32 (9 with vel),
 *             scores [B, T * P] in_dtype, labels [B, T * P] int32 = class within the task + sum of the earlier
 *             tasks' ncls, counts [B] int32; rows at or beyond counts[b] are zero.  P = post_max_size.
 * Limits: 1 <= T <= 8, 1 <= ncls[t] <= 4, ncls * H * W < 2^31, K <= 1024, 1 <= post_max_size <= max_num.  Every
 * argument is checked before any device work.  Four launches on `stream`, no host synchronisation, no atomics
 * beyond integer LDS counts: the output is a pure function of the inputs, and the call can be captured in a
 * graph.  The workspace (vamp_det_workspace_bytes) needs no initialisation.
 * -------------------------------------------------------------------------- */
enum { VAMP_NMS_CIRCLE = 0, VAMP_NMS_SIZE_AWARE = 1, VAMP_NMS_ROTATE = 2 };
typedef struct VampDetTask {
  const void* heatmap;
  const void* reg;
  const void* height;
  const void* dim;
  const void* rot;
  const void* vel;       /* NULL without velocity */
} VampDetTask;
typedef struct VampDetDesc {
  int32_t B, T, H, W;
  int32_t ncls[8];
  int32_t max_num, pre_max_size, post_max_size;
  int32_t nms_kind;               /* VAMP_NMS_CIRCLE | VAMP_NMS_SIZE_AWARE | VAMP_NMS_ROTATE */
  int32_t in_dtype;               /* VAMP_F32 | VAMP_BF16 | VAMP_F16 */
  int32_t has_vel, norm_bbox;
  int32_t use_score_threshold, use_center_range;
  float score_threshold;
  float out_size_factor, voxel_size[2], pc_range[2];
  float post_center_range[6];
  float min_radius[8], thresh_scale[8], nms_thr[8];
  int32_t reserved;               /* 0 */
} VampDetDesc;
size_t vamp_det_workspace_bytes(const VampDetDesc* d);
int vamp_det_postprocess(const VampDetDesc* d, const VampDetTask* tasks, float* boxes, void* scores, int32_t* labels,
                         int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Detection training targets: the reference head's get_targets (bev_depth_head.py:168-319, with mmdet3d's
 * gaussian_radius and draw_heatmap_gaussian) for all T tasks of a head and all B samples, on the device.
 * Inputs: boxes [B, M, box_cols] fp32 (x y z dx dy dz yaw [vx vy]) and labels [B, M] (label_dtype) of flat class
 * ids; rows past a sample's count carry label -1.  Task t owns the labels flag_t .. flag_t + ncls[t] - 1, flag_t
 * the sum of the earlier tasks' ncls; other labels (-1, >= the sum, ...) belong to no task.
 *
 *  slots      per (sample, task) the task's boxes class by class in class order, ascending box index within a
 *             class (the order of torch.where); slot k is the position in that run, only k < max_objs counts.
 *  size       w = box[3] * (1 / voxel_size[0]) * (1 / out_size_factor), l likewise with box[4] and voxel_size[1]
 *             (aten divides by a CPU scalar as a product with its reciprocal: 1.0f / b for the fp32 voxel size,
 *             (float) (1.0 / b) for a Python number; each op rounded, no FMA); the box is skipped unless w > 0
 *             and l > 0 (a NaN fails).
 *  radius     r = max(min_radius, int(gaussian_radius((l, w), gaussian_overlap))), the three roots in fp32 op by
 *             op with the Python-float terms of the overlap rounded to fp32; a radius that is not finite or is
 *             >= 2^30 (where the reference raises) skips the box.
 *  centre     c = (xy - pc_range) * (1 / voxel_size) * (1 / out_size_factor) in fp32, cast to int32 as aten does
 *             on this device (truncation, NaN -> 0); the box is skipped unless 0 <= x < fw and 0 <= y < fh.
 *  heatmap    max-merge of the stamp exp(-(dx^2 + dy^2) / ((2 sigma) sigma)), sigma = (2 r + 1) / 6, in float64,
 *             zeroed below DBL_EPSILON, rounded to fp32, over |dx| <= r, |dy| <= r clipped to the map.
 *  rows       anno [k] = (cx - x, cy - y, z, dims (log when norm_bbox), sin yaw, cos yaw[, vx, vy]), ind [k] =
 *             y * fw + x, mask [k] = 1; skipped slots and slots past the task's count are zero.
 * Outputs: heatmaps, task-major: task t's [B, ncls[t], fh, fw] block follows the earlier tasks' (each a
 * contiguous view); anno [T, B, max_objs, code] fp32, inds [T, B, max_objs] int64, masks [T, B, max_objs]
 * uint8.  Every element is written.
 * Limits: 1 <= B <= 4096, 1 <= T <= 8, 1 <= ncls[t] <= 4, 0 <= M <= 2^20, box_cols 7 | 9 with code = box_cols + 1,
 * 1 <= max_objs <= 8192, 1 <= fh, fw <= 8192, out_size_factor >= 1, voxel_size > 0.  Every argument is checked
 * before any device work.  Two launches on `stream`, no host synchronisation, no atomics: the output is a pure
 * function of the inputs, and the call can be captured in a graph.  The workspace
 * (vamp_det_targets_workspace_bytes) needs no initialisation.
 * -------------------------------------------------------------------------- */
typedef struct VampDetTargetDesc {
  double gaussian_overlap;        /* train_cfg['gaussian_overlap'], the Python float */
  int32_t B, T, M;
  int32_t ncls[8];
  int32_t box_cols;               /* 7 | 9 */
  int32_t code;                   /* anno width, len(code_weights): box_cols + 1 */
  int32_t max_objs;               /* max_objs * dense_reg */
  int32_t fh, fw;                 /* grid_size[1] // out_size_factor, grid_size[0] // out_size_factor */
  int32_t out_size_factor;
  int32_t min_radius;
  int32_t norm_bbox;
  int32_t label_dtype;            /* VAMP_I32 | VAMP_I64 */
  float voxel_size[2], pc_range[2];
  int32_t reserved[2];            /* 0 */
} VampDetTargetDesc;
size_t vamp_det_targets_workspace_bytes(const VampDetTargetDesc* d);
int vamp_det_targets(const VampDetTargetDesc* d, const float* boxes, const void* labels, float* heatmaps, float* anno,
                     int64_t* inds, uint8_t* masks, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Detection loss: the reference head's loss (bev_depth_head.py:321-379 -- clip_sigmoid and GaussianFocalLoss on
 * the heatmaps, code-weighted L1 on the box rows gathered at the targets' cells) for all T tasks of a head, forward
 * and gradient, on the device.  fp32 predictions only (the head runs under autocast(False), bev_depth_head.py:140).
 * Inputs: per task a VampDetTask of contiguous fp32 tensors (heatmap [B, ncls[t], H, W], reg [B, 2, H, W], height
 * [B, 1, H, W], dim [B, 3, H, W], rot [B, 2, H, W], vel [B, 2, H, W] or NULL) and the packed targets of
 * vamp_det_targets: heat (task t's [B, ncls[t], H, W] block after the earlier tasks'), anno [T, B, max_objs, code]
 * fp32, inds [T, B, max_objs] int64, masks [T, B, max_objs] uint8.  code is 10 with vel and 8 without; its columns
 * map to reg, height, dim, rot, vel in that order.
 *
 *  counts     counts[t] = (number of heat elements equal to 1, sum of masks) as fp32, unclamped (a caller may
 *             average them over ranks).  Where they are used: f_pos = max(counts[t][0], 1), f_num =
 *             max(counts[t][1], 1e-4).
 *  heatmap    s = sigmoid(x), p = clamp(s, 1e-4, 1 - 1e-4), pos = -log(p + 1e-12) (1 - p)^2 [h == 1], neg =
 *             -log(1 - p + 1e-12) p^2 (1 - h)^4, every step one fp32 operation in torch's order; L_heat[t] =
 *             sum(pos + neg) / f_pos, the sum taken in float64.
 *  boxes      slot (b, k) is live when masks[t, b, k] != 0 and 0 <= inds[t, b, k] < H W; a masked slot whose index
 *             is out of range is skipped and never dereferenced (torch's gather would assert there).  Column c is
 *             live when anno[t, b, k, c] is not NaN.  L_box[t] = loss_bbox_weight * sum over live slots and
 *             columns of code_weights[c] |pred[b, c, ind] - anno| / f_num, the sum in float64.
 *  loss       loss[0] = sum over t of (L_heat[t] + L_box[t]); terms [T, 2] = (L_heat, L_box) per task.
 *  gradient   scaled by the device scalar grad_loss[0].  Heatmap: grad_loss / f_pos [1e-4 <= s <= 1 - 1e-4]
 *             s (1 - s) ([h == 1] (-(1 - p)^2 / (p + 1e-12) + 2 (1 - p) log(p + 1e-12)) + (1 - h)^4 (p^2 /
 *             (1 - p + 1e-12) - 2 p log(1 - p + 1e-12))), s and p recomputed from the logits.  Boxes: grad_loss
 *             loss_bbox_weight code_weights[c] sign(pred - anno) / f_num (sign(0) = 0) at (b, c, ind) for every
 *             live slot and column; live slots of one (t, b) that share a cell are summed in ascending slot
 *             order by one writer.  Every other element of every gradient map is written as zero: the call owns
 *             the whole buffers.  `grads` is a VampDetTask table of the outputs; a NULL entry is not computed.
 * Sums run in a fixed order (float64 partials per workgroup in the workspace, added by one workgroup of a second
 * launch): results are bitwise repeatable.  No float atomics, no host synchronisation; vamp_det_loss_counts is one
 * launch, forward and backward two each, all capturable in a graph.  Limits: 1 <= B <= 4096, 1 <= T <= 8,
 * 1 <= ncls[t] <= 4, 1 <= H, W <= 8192, 1 <= max_objs <= 4096 (the backward looks for shared cells in time
 * quadratic in the live slots of a sample and task), code 8 | 10 agreeing with has_vel.  A bad descriptor returns VAMP_EINVAL (and a
 * workspace size of 0), a NULL pointer or a workspace that is too small VAMP_ENOSPC, both before any launch.  The
 * workspace (vamp_det_loss_workspace_bytes, one size for forward and backward) needs no initialisation.
 * -------------------------------------------------------------------------- */
typedef struct VampDetLossDesc {
  int32_t B, T, H, W;
  int32_t ncls[8];
  int32_t code;                   /* 10 with vel, 8 without */
  int32_t max_objs;               /* slots per (task, sample) */
  int32_t has_vel;
  float code_weights[10];         /* train_cfg['code_weights'] */
  float loss_bbox_weight;
  int32_t reserved[2];            /* 0 */
} VampDetLossDesc;
size_t vamp_det_loss_workspace_bytes(const VampDetLossDesc* d);
int vamp_det_loss_counts(const VampDetLossDesc* d, const float* heat, const uint8_t* masks, float* counts,
                         void* stream);
int vamp_det_loss_forward(const VampDetLossDesc* d, const VampDetTask* preds, const float* heat, const float* anno,
                          const int64_t* inds, const uint8_t* masks, const float* counts, float* loss, float* terms,
                          void* workspace, size_t workspace_bytes, void* stream);
int vamp_det_loss_backward(const VampDetLossDesc* d, const VampDetTask* preds, const float* heat, const float* anno,
                           const int64_t* inds, const uint8_t* masks, const float* counts, const float* grad_loss,
                           const VampDetTask* grads, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Rgb loss (base_exp.py:286, 539-549): mean smooth-L1 (beta 1) + 1 - MS-SSIM of the rendered image `pred` against
 * the label `target`, both [N, C, H, W] fp32 and contiguous (N = batch x cameras), and its gradient with respect to
 * pred.  MS-SSIM is MultiScaleStructuralSimilarityIndexMeasure(data_range) with its defaults: a Gaussian window of
 * 11 taps, sigma 1.5, normalised, applied as a valid correlation (separably: it is the outer product of the 1-D
 * window); five scales with betas 0.0448, 0.2856, 0.3001, 0.2363, 0.1333; c1 = (k1 data_range)^2, c2 = (k2
 * data_range)^2.
 *
 *  per scale  mux, muy, sxx = E[xx] - mux^2, syy, sxy = E[xy] - mux muy (window sums and differences in float64),
 *             cs = (2 sxy + c2) / (sxx + syy + c2); on the last scale cs is multiplied by l = (2 mux muy + c1) /
 *             (mux^2 + muy^2 + c1).  v[n, i] = relu(mean over C and the valid region), the sum in float64.  Between
 *             scales x and y are 2x2 average-pooled with floor: an odd last row or column is dropped.
 *  loss       ms_ssim = mean over n of PROD_i v[n, i]^beta_i; terms = (mean smooth-L1, ms_ssim); loss[0] = terms[0]
 *             + 1 - terms[1]; vals [N, 5] = v.
 *  gradient   grad_pred = grad_loss[0] (a device scalar) times d loss / d pred, every element written once.
 *             Where some v[n, i] is 0 after the relu (an anti-correlated prediction), image n contributes 0 to
 *             ms_ssim and its MS-SSIM gradient is DEFINED as exactly 0; its smooth-L1 gradient is unaffected.  This
 *             is the one difference from the torch expression, which yields NaN there (relu(v) ** beta has the
 *             gradient inf * 0; a relu backward that selects instead of multiplying may drop the NaN again).
 * Forward: one launch per scale (float64 partials per workgroup into the workspace, the pooled images of the next
 * scale, the per-pixel unit adjoints the backward applies the transposed window to) and one finishing workgroup
 * that adds the partials in a fixed order.  Backward: one launch per scale, coarse to fine; it takes the workspace
 * as the forward of the same inputs left it.  No float atomics, no host synchronisation, bitwise repeatable,
 * capturable in a graph.  The workspace (8-byte aligned, vamp_rgb_loss_workspace_bytes: about 16 bytes per valid
 * pixel and 4 per pixel over all scales) needs no initialisation.  Limits: N >= 1, 1 <= C <= 4, 176 <= H, W <= 16384
 * (the fifth scale still holds one window), N C H W < 2^31.  A bad descriptor returns VAMP_EINVAL (and a workspace
 * size of 0), a NULL pointer or a workspace that is too small VAMP_ENOSPC, both before any launch.
 * -------------------------------------------------------------------------- */
typedef struct VampRgbLossDesc {
  int32_t N, C, H, W;
  float data_range;               /* 1.0 */
  float k1, k2;                   /* 0.01, 0.03 */
} VampRgbLossDesc;
size_t vamp_rgb_loss_workspace_bytes(const VampRgbLossDesc* d);
int vamp_rgb_loss_forward(const VampRgbLossDesc* d, const float* pred, const float* target, float* loss, float* terms,
                          float* vals, void* workspace, size_t workspace_bytes, void* stream);
int vamp_rgb_loss_backward(const VampRgbLossDesc* d, const float* pred, const float* target, const float* grad_loss,
                           float* grad_pred, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Segmentation loss (base_exp.py:519-575: the camera, BEV, lidar-point and occupancy segmentation terms of the
 * training step, each F.cross_entropy(x[mask], y[mask]) + lovasz_softmax(F.softmax(x[mask], 1), y[mask]);
 * lovasz_losses.py:171-199, lovasz_softmax_flat with classes='present'): loss = w_ce CE + w_lv LV over the VALID
 * elements -- mask byte set (mask may be NULL: all) and label in [0, C) -- and its gradient with respect to the
 * logits, without compacting the inputs.  Logits are fp32 in the layouts of vamp_confusion_update (VAMP_SEG_ROWS
 * [n, C], VAMP_SEG_PLANES [B, C, S], element i = b * S + s), labels [n] of label_dtype, mask [n] bool bytes.
 *
 *  CE         -(1 / n) sum over valid i of log softmax(logits[i])[labels[i]]; n = number of valid elements.
 *  LV         p = softmax in fp32, err[i, c] = |[labels[i] == c] - p[i, c]| in fp32.  For every class with a valid
 *             foreground element: the valid elements sorted by err descending, bit-equal errors by ascending element
 *             index (a total order: the permutation is unique), and sum_k err_k delta_k with the Jaccard step from
 *             integer counts in float64 -- G foreground elements, cum_k of them among the first k, I = G - cum_k,
 *             U = G + k - cum_k: delta_k = 1 / U at a foreground element, I / ((U - 1) U) at a background one.
 *             LV = mean over those classes.
 *  outputs    loss [1], terms [2] = (CE, LV), counts [2] int32 = (n, classes present).  sorted_err / perm (each
 *             NULL or [C, B S] fp32 / int32, class-major) receive, for EVERY class, the sorted errors and element
 *             indices of the valid elements in a row's first n entries; the rest of a row is unspecified.
 *  gradient   grad_logits (the logits' layout, every element written once) = grad_loss[0] (a device scalar, the
 *             last factor) times w_ce (p - fg) / n + w_lv p (u - sum_k p_k u_k) / present, u[i, c] = -sign(fg - p)
 *             delta_rank(i, c) for present classes (sign(0) = 0), else 0.  Invalid elements get exactly 0.
 *  n = 0      loss, terms and the whole gradient are DEFINED as exactly 0: the one difference from the torch
 *             expression, whose cross_entropy of an empty selection is NaN.
 * Forward: one pass over the rows, a per-class LSD radix sort (four 8-bit passes of histogram, scan, stable
 * scatter), a foreground scan of the sorted order, and one finishing workgroup that adds the float64 partials in a
 * fixed order -- sixteen launches whose grids depend on the shapes only.  Backward: one launch; it reads `kept`
 * (vamp_seg_loss_kept_bytes: 4 bytes per element and class, the unit gradients u) as the forward of the same
 * inputs left it.  The workspace (vamp_seg_loss_workspace_bytes, about 17 bytes per element and class) is needed
 * by the forward only.  Neither needs initialisation; both must be 8-byte aligned.  No float atomics, no host
 * synchronisation, bitwise repeatable, capturable in a graph.  Limits: 2 <= C <= 32, B S >= 1, B S C < 2^31.
 * A bad descriptor returns VAMP_EINVAL (and a size of 0), a NULL required pointer or a buffer that is too small
 * VAMP_ENOSPC, both before any launch.
 * -------------------------------------------------------------------------- */
typedef struct VampSegLossDesc {
  int64_t B, S;                   /* n = B * S elements (ROWS: B = 1) */
  int32_t C;                      /* classes */
  int32_t layout;                 /* VAMP_SEG_ROWS | VAMP_SEG_PLANES */
  int32_t label_dtype;            /* VAMP_I64 | VAMP_I32 | VAMP_U8 */
  int32_t reserved;               /* 0 */
  float w_ce, w_lv;
} VampSegLossDesc;
size_t vamp_seg_loss_workspace_bytes(const VampSegLossDesc* d);
size_t vamp_seg_loss_kept_bytes(const VampSegLossDesc* d);
int vamp_seg_loss_forward(const VampSegLossDesc* d, const float* logits, const void* labels, const uint8_t* mask,
                          float* loss, float* terms, int32_t* counts, float* sorted_err, int32_t* perm, void* kept,
                          size_t kept_bytes, void* workspace, size_t workspace_bytes, void* stream);
int vamp_seg_loss_backward(const VampSegLossDesc* d, const float* logits, const void* labels, const uint8_t* mask,
                           const float* grad_loss, float* grad_logits, const void* kept, size_t kept_bytes,
                           void* stream);

/* --------------------------------------------------------------------------
 * Masked regression losses (the regression terms of the training step: base_exp.py:588-594 get_depth_loss,
 * F.smooth_l1_loss(depth_p[fg], depth_l[fg]); :581-586 get_height_loss_bev, the same under bev_mask; :533-537
 * get_sdf_loss, the mean of (sdf - sdf_bias)^2; :523-531 get_occ_density_loss, F.mse_loss under mask_camera and,
 * from a second call, under ~mask_camera).  One call evaluates a PACK of 1 <= T <= 8 terms in two launches, and the
 * gradients of the whole pack in one, without compacting anything.  Term t:
 *
 *  inputs     pred [n] contiguous, fp32 or bf16 (pred_dtype), read in place; target [n] fp32, or the constant
 *             target_value when target_is_const is 1 (the target pointer is then ignored); mask [n] bool bytes or
 *             NULL.  The pointers may have any element offset (16-byte loads are used where all of a term's are
 *             aligned for them; the results do not depend on it).
 *  element    d = float(pred) - target and the element loss in fp32 as aten rounds them: VAMP_REG_SMOOTH_L1 (beta 1)
 *             z = |d|, z < 1 ? (0.5 z) z : z - 0.5; VAMP_REG_MSE d d.
 *  loss       S1 = the elements whose mask byte is set (all of them without a mask), S0 the others; mean_k = the
 *             float64 sum over S_k divided by |S_k|.  losses[t] = mean_1 (VAMP_REG_SET), mean_0 (VAMP_REG_CLEAR) or
 *             mean_1 + mean_0 (VAMP_REG_BOTH), rounded to fp32 once; counts[t] = (|S1|, |S0|) int64.  CLEAR and BOTH
 *             need a mask.  Elements are selected, not weighted: a NaN or an infinity in pred or target outside the
 *             selected side(s) reaches neither the loss nor a gradient.
 *  |S_k| = 0  mean_k is DEFINED as exactly 0 (and there is no element to receive a gradient from it): the one
 *             difference from the torch expressions, whose mean of an empty selection is NaN.
 *  gradient   grad_pred[t] [n] of pred's dtype, every element written once: grad_losses[t] l'(d) / |S_k| at an
 *             element of a selected side k (l' = d where |d| < 1, else sign(d), a NaN d stays NaN as in aten; 2 d for
 *             the squared error), formed in
 *             float64 and rounded once to fp32 (from there to nearest-even bf16), exactly 0 elsewhere.  A NULL entry
 *             of grad_pred_host skips the term.  `counts` is the forward's output, read on the device.  No gradient
 *             goes to target.
 * pred_host, target_host, mask_host and grad_pred_host are HOST arrays of T device pointers, read before the call
 * returns.  Forward: reg_partial_kernel (term t owns ceil(n / VAMP_REG_TILE) consecutive workgroups; float64 sums
 * and integer counts per workgroup into the workspace) and one finishing workgroup that adds a term's partials in
 * index order.  The workspace (8-byte aligned, vamp_reg_loss_workspace_bytes: 24 bytes per workgroup) is forward
 * scratch and needs no initialisation.  No atomics, no host synchronisation, bitwise repeatable, capturable in a
 * graph; a term's results do not depend on the other terms of the pack.  Limits: 1 <= T <= 8, 1 <= n < 2^31.
 * Everything that is refused -- T, n, kind, side, pred_dtype or target_is_const out of range, CLEAR or BOTH without
 * a mask, a NULL required pointer, a workspace that is too small -- returns VAMP_EINVAL (and a size of 0) before any
 * launch.
 * -------------------------------------------------------------------------- */
#define VAMP_REG_MAX_TERMS 8
#define VAMP_REG_TILE 4096        /* elements per workgroup */
enum { VAMP_REG_SMOOTH_L1 = 0, VAMP_REG_MSE = 1 };
enum { VAMP_REG_SET = 0, VAMP_REG_CLEAR = 1, VAMP_REG_BOTH = 2 };
typedef struct VampRegTerm {
  int64_t n;                      /* elements */
  int32_t kind;                   /* VAMP_REG_SMOOTH_L1 | VAMP_REG_MSE */
  int32_t side;                   /* VAMP_REG_SET | VAMP_REG_CLEAR | VAMP_REG_BOTH */
  int32_t pred_dtype;             /* VAMP_F32 | VAMP_BF16 */
  int32_t target_is_const;        /* 1: the target is target_value */
  float target_value;
  int32_t reserved;               /* 0 */
} VampRegTerm;
typedef struct VampRegLossDesc {
  int32_t T;                      /* terms in use */
  int32_t reserved;               /* 0 */
  VampRegTerm terms[VAMP_REG_MAX_TERMS];
} VampRegLossDesc;
size_t vamp_reg_loss_workspace_bytes(const VampRegLossDesc* d);
int vamp_reg_loss_forward(const VampRegLossDesc* d, const void* const* pred_host, const float* const* target_host,
                          const uint8_t* const* mask_host, float* losses, int64_t* counts, void* workspace,
                          size_t workspace_bytes, void* stream);
int vamp_reg_loss_backward(const VampRegLossDesc* d, const void* const* pred_host, const float* const* target_host,
                           const uint8_t* const* mask_host, const int64_t* counts, const float* grad_losses,
                           void* const* grad_pred_host, void* stream);

/* --------------------------------------------------------------------------
 * The parameter update that ends a training step (base_cli.py:61-90 Trainer(gradient_clip_val=35, precision=16);
 * base_exp.py:931-943 AdamW(lr, weight_decay=1e-7); callbacks/ema.py:23-117 ModelEMA / EMACallback): unscale and clip
 * the gradients by their global norm, AdamW, the averaged (EMA) weights of every floating-point state entry and the
 * dynamic loss scale, for any number of tensors in three launches.
 *
 *  table      device array of n_param_chunks + n_buffer_chunks VampUpdateChunk, built once by the host: every tensor
 *             cut into chunks of at most VAMP_UPDATE_CHUNK elements, a chunk never crossing a tensor; the chunks of
 *             the parameters first, those of the buffers (EMA only) behind them.  `param` and `grad` point at the
 *             chunk's first element (fp32, contiguous, any element alignment: 16-byte accesses are used where both are
 *             aligned for them, the results do not depend on it); state_off is the chunk's element offset in the flat
 *             state arrays, a multiple of 4; kind VAMP_UPDATE_PARAM, or VAMP_UPDATE_EMA_ONLY for a buffer and for a
 *             parameter that has no gradient in this step (grad NULL).
 *  state      exp_avg, exp_avg_sq (covering the parameters' state offsets) and ema (covering all), flat fp32 arrays,
 *             16-byte aligned, in which every tensor starts at a multiple of 4 elements and is padded to one.
 *  scalars    one VampUpdateScalars in device memory.  The caller initialises lr, step (t), updates (n), scale (S, 1
 *             without loss scaling) and growth; the call advances the counters and fills in the rest, so a replayed
 *             graph keeps counting.  t advances unless found_inf; n always advances.
 *  norm       total_norm = sqrt(sum g g) / S over the parameters with a gradient, the sum in float64 in a fixed
 *             order; found_inf = the sum is not finite (exactly: some gradient element is inf or NaN).
 *  clip       clip_coef = min(1, max_norm / (total_norm + 1e-6)), 1 when max_norm <= 0; mult = clip_coef / S.
 *  element    in fp32, each operation rounded by itself: g' = g mult; p = p (1 - lr wd); m = m + (g' - m)(1 - beta1);
 *             v = v beta2 + ((1 - beta2) g') g'; p = p - (lr / bc1)(m / (sqrt(v) / sqrt(bc2) + eps));
 *             e = e d + (1 - d) p with d = ema_decay (1 - exp(-n / 2000)).  The scalars are formed in float64 and
 *             rounded to fp32 once.  With found_inf set p, m and v keep their bits and the EMA line runs on the
 *             unchanged p.  A VAMP_UPDATE_EMA_ONLY chunk takes the EMA line only; with ema_decay <= 0 there is no
 *             EMA, ema may be NULL and the buffer chunks are not visited.
 *  scale      VAMP_UPDATE_SCALE_DYNAMIC: S x 0.5 on found_inf, x 2 after VAMP_UPDATE_GROWTH_INTERVAL steps without
 *             one (torch.amp.GradScaler's rule); otherwise S is left as it is.
 * The workspace (8-byte aligned, vamp_param_update_workspace_bytes: 8 bytes per parameter chunk) needs no
 * initialisation.  No atomics, no host synchronisation, bitwise repeatable, capturable in a graph; grids depend on
 * the chunk counts only.  A bad descriptor (no chunks, a beta outside [0, 1), ...), a NULL table, scalar block or
 * required state array return VAMP_EINVAL (and a size of 0), a workspace that is too small VAMP_ENOSPC, all before
 * any launch.  The library keeps no state between calls.
 * -------------------------------------------------------------------------- */
#define VAMP_UPDATE_CHUNK 4096    /* elements per workgroup */
#define VAMP_UPDATE_GROWTH_INTERVAL 2000
enum { VAMP_UPDATE_PARAM = 0, VAMP_UPDATE_EMA_ONLY = 1 };
enum { VAMP_UPDATE_SCALE_NONE = 0, VAMP_UPDATE_SCALE_STATIC = 1, VAMP_UPDATE_SCALE_DYNAMIC = 2 };
typedef struct VampUpdateChunk {
  void* param;                    /* the chunk's first element of the parameter or buffer */
  const void* grad;               /* the same element of the gradient; NULL for VAMP_UPDATE_EMA_ONLY */
  int64_t state_off;              /* element offset in exp_avg / exp_avg_sq / ema, a multiple of 4 */
  int32_t len;                    /* 1 .. VAMP_UPDATE_CHUNK */
  int32_t kind;                   /* VAMP_UPDATE_PARAM | VAMP_UPDATE_EMA_ONLY */
} VampUpdateChunk;
typedef struct VampUpdateScalars {
  double lr;                      /* in */
  int64_t step;                   /* in, out: t, optimizer steps taken */
  int64_t updates;                /* in, out: n, EMA updates made */
  float scale;                    /* in, out: the loss scale S the gradients carry; afterwards the next one */
  int32_t growth;                 /* in, out: steps since the scale last changed */
  int32_t found_inf;              /* out */
  float total_norm, clip_coef, mult;          /* out */
  float decay_mul, step_size, bc2_sqrt;       /* out: 1 - lr wd, lr / (1 - beta1^t), sqrt(1 - beta2^t) */
  float ema_d, ema_1md;                       /* out: d, 1 - d */
  int32_t reserved[15];
} VampUpdateScalars;
typedef struct VampParamUpdateDesc {
  double beta1, beta2, eps, weight_decay;
  double max_norm;                /* <= 0: no clipping (the norm is still computed) */
  double ema_decay;               /* <= 0: no EMA */
  int32_t n_param_chunks, n_buffer_chunks;
  int32_t scale_mode;             /* VAMP_UPDATE_SCALE_* */
  int32_t reserved;               /* 0 */
} VampParamUpdateDesc;
size_t vamp_param_update_workspace_bytes(const VampParamUpdateDesc* d);
int vamp_param_update_step(const VampParamUpdateDesc* d, const void* table, float* exp_avg, float* exp_avg_sq,
                           float* ema, void* scalars, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Camera and BEV training labels rasterised from the lidar points: the reference loader's depth_transform
 * (nusc_det_seg_dataset.py:178-231) behind the margins of map_pointcloud_to_image (:362-367), get_bev_seg_map
 * (:233-265) and the every-s-th-pixel pick of get_downsampled_gt (base_exp.py:596-632), for all B samples and N
 * cameras on the device.
 * Inputs: points [B, M, point_cols] fp32 (x y z [intensity]) in the bda-augmented ego frame, labels [B, M]
 * (label_dtype), counts [B] int32 (rows i >= counts[b] of sample b do nothing; NULL: all M rows count), lidar2cam
 * [B, N, 4, 4] fp32 (points to camera frame), intrin [B, N, 4, 4] fp32, aug [B, N, 8] float64 in DEVICE memory:
 * resize, crop_x, crop_y, flip (0 | 1), cos, sin of the rotation, 0, 0 -- so the augmentation can change under a
 * replayed graph.
 *
 *  camera     per camera, every step one fp32 operation in this order (no FMA):
 *    frame    xc = ((m00 x + m01 y) + m02 z) + m03, yc and zc likewise with rows 1 and 2 of lidar2cam; depth = zc.
 *    pixel    u = ((k00 xc + k01 yc) + k02 zc) / ((k20 xc + k21 yc) + k22 zc), v likewise with row 1 of intrin.
 *    margins  keep iff depth > 0, u > 1, u < raw_w - 1, v > 1, v < raw_h - 1 (:362-367).
 *    augment  u *= (float) resize, v *= (float) resize; u -= crop_x, v -= crop_y; flip: u = W - u; u -= W / 2,
 *             v -= H / 2; rotation in float64 as numpy's matmul computes it, u' = cos u + sin v, v' = -sin u + cos v,
 *             each rounded to fp32; u += W / 2, v += H / 2 (:193-211).
 *    valid    iff 0 <= u < W and 0 <= v < H, tested on the floats before any conversion (NaN, +-Inf, 1e30 and
 *             -0.5, which would truncate to 0, fall out); the pixel (iv, iu) is the truncation of (v, u).
 *    stride   the point is dropped unless iu % stride == 0 and iv % stride == 0; the cell is (iv / stride,
 *             iu / stride): exactly map[::stride, ::stride] of the full-resolution map.
 *    winner   the smallest depth (:225 sorts by -depth, the last write wins); equal depths go to the LOWEST point
 *             index.  The reference's order among equal depths is that of an unstable argsort, i.e. undefined: the
 *             tie rule is this library's.  key = (bits(depth) << 32) | index under a 64-bit unsigned atomic min.
 *  BEV        coordinates in float64 as numpy makes them: cx = ((double) x - origin_x) / size, cy likewise, origin =
 *             bound_lo - size / 2 computed by the caller; keep iff cx > 1, cx < nx - 1, cy > 1, cy < ny - 1, z > z_lo
 *             and z < z_hi (the z comparison in fp32); the cell is (trunc(cy), trunc(cx)); the largest z wins (:258
 *             sorts by height, the last write wins), equal heights go to the lowest index (ours again; -0.0 ranks
 *             below +0.0).  key = (ordered(z) << 32) | (0xFFFFFFFF - index) under a 64-bit unsigned atomic max,
 *             ordered the monotone map of fp32 bits to uint32; key 0 is an empty cell.
 *             The map is [ny, nx], rows along y, columns along x.  That equals the reference for its square grids;
 *             its own indexing (a map shaped by (x, y) written at [y, x]) is inconsistent when nx != ny.
 * Outputs, every element written: cam_depth [B, N, h, w] fp32 (the winner's depth bits, 0 when empty), cam_seg
 * [B, N, h, w] int64 (labels[winner] & 0xFF, 0 when empty), cam_fg [B, N, h, w] uint8 (depth > 0), h = H / stride,
 * w = W / stride; bev_seg [B, ny, nx] int64, bev_height [B, ny, nx] fp32 (0 when empty), bev_mask [B, ny, nx] uint8.
 * The three camera outputs may be NULL together and the three BEV outputs likewise: that part is skipped (and
 * lidar2cam, intrin, aug are not read without the camera part); both parts NULL is an error.
 * Limits: 1 <= B <= 4096, 1 <= N <= 16, 0 <= M <= 2^24, point_cols 3 | 4, label_dtype VAMP_U8 | VAMP_I64,
 * 1 <= H, W, ny, nx <= 8192, stride >= 1 dividing H and W, 1 <= raw_w, raw_h <= 65536, size > 0, z_lo < z_hi,
 * B N h w and B ny nx <= 2^33.  Every argument is checked before any device work: a failed check returns VAMP_EINVAL
 * (and a workspace size of 0) with a message, a workspace that is NULL or too small VAMP_ENOSPC.
 * Three launches on `stream` (fill, scatter with one thread per point, resolve with one thread per cell; no scatter
 * when M = 0), no host synchronisation, no float atomics: integer min / max do not depend on the arrival order, so
 * the output is a pure function of the inputs, bitwise repeatable, and the call can be captured in a graph.  The
 * workspace (16-byte aligned, vamp_lidar_labels_workspace_bytes: 8 bytes per cell of both parts) needs no
 * initialisation.
 * -------------------------------------------------------------------------- */
typedef struct VampLidarLabelDesc {
  double origin_x, origin_y;      /* BEV: bound_lo - size / 2 */
  double size;                    /* BEV cell size */
  int32_t B, N, M;
  int32_t point_cols;             /* 3 | 4 */
  int32_t label_dtype;            /* VAMP_U8 | VAMP_I64 */
  int32_t H, W;                   /* final_dim */
  int32_t stride;
  int32_t raw_w, raw_h;           /* the raw image the intrinsics belong to */
  int32_t ny, nx;
  float z_lo, z_hi;
  int32_t reserved[2];            /* 0 */
} VampLidarLabelDesc;
size_t vamp_lidar_labels_workspace_bytes(const VampLidarLabelDesc* d);
int vamp_lidar_labels(const VampLidarLabelDesc* d, const float* points, const void* labels, const int32_t* counts,
                      const float* lidar2cam, const float* intrin, const double* aug, float* cam_depth,
                      int64_t* cam_seg, uint8_t* cam_fg, int64_t* bev_seg, float* bev_height, uint8_t* bev_mask,
                      void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Camera images on the device: the reference loader's img_transform (nusc_det_seg_dataset.py:118-146: Pillow's
 * resize, crop, transpose(FLIP_LEFT_RIGHT) and rotate) followed by mmcv.imnormalize (:679-681), for all B samples and
 * N cameras, with the (resize, resize_dims, crop, flip, rotate) values of sample_ida_augmentation (:472-499).
 * For one raw RGB frame raw[raw_h, raw_w, 3] uint8, resize_dims = (newW, newH), crop = (x0, y0, x0 + W, y0 + H) and
 * final_dim = (H, W), rules 1 - 5 apply in this order.  Rules 1 - 4 restate Pillow's arithmetic and are pinned
 * byte for byte against Pillow 12.2.0 by tests/golden/camera_images.npz (the reference does not pin Pillow); rule 5
 * restates mmcv.imnormalize, and its parity with OpenCV is UNPINNED: neither OpenCV nor mmcv was at hand.
 *
 *  1 resize   Image.resize without a resample argument: bicubic, a = -0.5, two separable passes, horizontal first,
 *             with a uint8 image between them.  Per axis with sizes in -> out, in float64: scale = in / out,
 *             fs = max(scale, 1), support = 2 fs, ss = 1 / fs.  For output index i: c = (i + 0.5) scale,
 *             lo = max((int) (c - support + 0.5), 0), hi = min((int) (c + support + 0.5), in); the taps are
 *             k[j] = cubic((j + lo - c + 0.5) ss) for j < hi - lo, with cubic(x) = ((1.5 |x| - 2.5) |x|) |x| + 1 for
 *             |x| < 1, (((|x| - 5) |x| + 8) |x| - 4) (-0.5) for |x| < 2, else 0; they are divided by their sum, taken
 *             from left to right, and made fixed-point: ki = (int) (k 2^22 + 0.5) for k >= 0, (int) (k 2^22 - 0.5)
 *             for k < 0, (int) truncating.  A pass computes clip(0, 255, (2^21 + sum_j ki[j] pix[lo + j]) >> 22) per
 *             channel in int32 (255 sum |ki| stays below 2^31 for these taps), the shift arithmetic.
 *  2 crop     pixel (x, y) of the crop is resized pixel (x + x0, y + y0), 0 where that lies outside the resized
 *             image (y0 may be negative, x0 + W may exceed newW).
 *  3 flip     x -> W - 1 - x.
 *  4 rotate   Image.rotate(angle): nearest neighbour about the centre, no expand, zero fill.  In float64:
 *             a = -radians(angle mod 360), m = [round(cos a, 15), round(sin a, 15), 0, round(-sin a, 15),
 *             round(cos a, 15), 0], m[2] = m[0] (-W / 2) + m[1] (-H / 2) + W / 2, m[5] = m[3] (-W / 2) + m[4] (-H / 2)
 *             + H / 2; with FIX(v) = floor(v 65536 + 0.5): a0, a1, a3, a4 = FIX(m[0]), FIX(m[1]), FIX(m[3]), FIX(m[4]),
 *             a2 = FIX(m[2] + 0.5 m[0] + 0.5 m[1]), a5 = FIX(m[5] + 0.5 m[3] + 0.5 m[4]).  Output (x, y) takes source
 *             ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16), arithmetic shifts in int32, 0 where the source is
 *             outside W x H.  Angle 0 is the identity by the same formula.  |angle| < 45 is the caller's to keep
 *             (Pillow switches to transposes at multiples of 90).
 *  5 normalise out[c] = ((float) img[c'] - mean[c]) * std_inv[c], c' = 2 - c if to_rgb else c (OpenCV's BGR -> RGB swap
 *             applied to Pillow's RGB image: a quirk of the reference, kept), std_inv[c] = (float) (1 / (double) std[c])
 *             computed by the caller; one fp32 rounding per operation, no fused multiply-add; planar [3, H, W].
 *
 * All float64 work is the caller's: the kernels read int32 plan tables in DEVICE memory, so the augmentation can
 * change under a replayed graph.  Per (b, n), for only the W resized columns and H resized rows the crop window
 * touches:
 *   col_first, col_count [B, N, W], col_taps [B, N, taps_x, W]: lo, hi - lo and ki of resized column x0 + x (tap-major);
 *              count 0 for a column outside the resized image; row_first, row_count [B, N, H], row_taps [B, N, taps_y, H]
 *              likewise for resized row y0 + y.
 *   consts     [B, N, VAMP_IMG_CONST_COLS]: a0 .. a5, x0, y0, newW, newH, flip (0 | 1), zeros (the kernels read a0 .. a5
 *              and flip; the crop is in the tables).
 * Range: at most VAMP_IMG_MAX_TAPS = 16 taps per output (scale = in / out up to about 3.7 per axis, i.e. resize down
 * to about 0.27; the reference draws 0.386 .. 0.55 and evaluates at 0.44; resize above 1 keeps support 2 and 4 - 5
 * taps), and a raw footprint of at most VAMP_IMG_FOOT_W x VAMP_IMG_FOOT_H pixels under any VAMP_IMG_TILE_H x
 * VAMP_IMG_TILE_W tile of the crop window; the descriptor carries the plan's tap capacities (the tables' strides) and
 * its largest footprint, and a plan beyond the range is refused.  The kernels clamp every window to the raw image and
 * to the footprint, so no table content can make them read or write out of bounds.
 * Inputs: raw uint8, element (b, n, y, x, c) at raw + b raw_b_stride + n raw_n_stride + y raw_row_stride + 3 x + c
 * (any row alignment).  Outputs, every element written: out [B, N, 3, H, W] fp32 | bf16 (round-to-nearest-even of the
 * fp32 value), 16-byte aligned, NULL with out_dtype VAMP_IMG_OUT_NONE; out_u8 [B, N, H, W, 3], the image of rule 4,
 * 4-byte aligned, or NULL; at least one of the two.
 * Limits: 1 <= B <= 4096, 1 <= N <= 16, B N <= 65535, 1 <= raw_h, raw_w <= 65536, 1 <= H, W <= 4096.  Every argument
 * is checked before any device work: a failed check returns VAMP_EINVAL (and a workspace size of 0) with a message, a
 * workspace that is NULL or too small VAMP_ENOSPC.  Two launches on `stream` (resample: footprint to LDS, horizontal
 * pass to a uint8 LDS tile, vertical pass to a uint8 staging image in the workspace; finish: rotate, flip, normalise),
 * no atomics, no host synchronisation, bitwise repeatable, capturable in a graph.  The workspace (16-byte aligned,
 * B N H align16(3 W) bytes) needs no initialisation.
 * -------------------------------------------------------------------------- */
#define VAMP_IMG_MAX_TAPS 16
#define VAMP_IMG_TILE_W 64
#define VAMP_IMG_TILE_H 8
#define VAMP_IMG_FOOT_W 272
#define VAMP_IMG_FOOT_H 48
#define VAMP_IMG_CONST_COLS 16
#define VAMP_IMG_OUT_NONE (-1)
typedef struct VampImageDesc {
  int64_t raw_b_stride, raw_n_stride, raw_row_stride;   /* bytes */
  int32_t B, N;
  int32_t raw_h, raw_w;
  int32_t H, W;                   /* final_dim */
  int32_t taps_x, taps_y;         /* tap capacity of col_taps / row_taps, 1 .. VAMP_IMG_MAX_TAPS */
  int32_t foot_w, foot_h;         /* the plan's largest raw footprint under one tile, 1 .. VAMP_IMG_FOOT_W / _H */
  int32_t out_dtype;              /* VAMP_F32 | VAMP_BF16 | VAMP_IMG_OUT_NONE */
  int32_t to_rgb;                 /* 0 | 1 */
  float mean[3], std_inv[3];
  int32_t reserved[2];            /* 0 */
} VampImageDesc;
size_t vamp_camera_images_workspace_bytes(const VampImageDesc* d);
int vamp_camera_images(const VampImageDesc* d, const uint8_t* raw, const int32_t* col_first, const int32_t* col_count,
                       const int32_t* col_taps, const int32_t* row_first, const int32_t* row_count,
                       const int32_t* row_taps, const int32_t* consts, void* out, uint8_t* out_u8, void* workspace,
                       size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------
 * Detection scoring, the per-batch half: what the reference leaves to the nuScenes devkit's NuScenesEval behind
 * src/evaluators/det_evaluators.py:61-117 (`_evaluate_single`; the attribute of a prediction is the speed rule of
 * :254-274, the class ranges, distance thresholds and the 2 m true-positive threshold are `detection_cvpr_2019`,
 * loaded at :50-55), fed by `test_step`'s get_bboxes results (src/exps/nuscenes/base_exp.py:665-746).  This is the
 * project's own restatement of the published protocol; parity with the devkit is unpinned.
 * Inputs: the detections of vamp_det_postprocess -- boxes [B, M, box_cols] fp32 (x y z dx dy dz yaw [vx vy]), scores
 * [B, M] (score_dtype), labels [B, M] int32, counts [B] int32 -- and the padded ground truth gt_boxes [B, G, box_cols]
 * fp32, gt_labels [B, G] (gt_label_dtype; a padding row carries -1), gt_attrs [B, G] int8 (index of the attribute name
 * or -1 for none; NULL with has_attrs 0: no ground truth has one).
 *
 *  filter     a box counts when sqrt(x^2 + y^2) < class_range[class], in float64 from the fp32 centre.
 *  order      per (sample, class) the surviving predictions by score descending, higher row first among equals.  -0
 *             equals +0; a NaN of either sign and any payload orders above every number (+inf included), and NaNs are
 *             equal among themselves: higher row first.  The record keeps the score's bits as they came.
 *  match      per distance threshold its own taken set: the prediction takes the nearest not yet taken ground truth of
 *             its class and sample (squared xy distance in float64, lowest row among equals) when that distance is
 *             strictly below the threshold, and is a false positive otherwise -- it never falls back to a farther one.
 *  errors     of the match at dist_th_tp, in float64, rounded to fp32: centre distance; 1 - IoU of the aligned sizes;
 *             |yaw difference| folded to period pi (VAMP_DET_EVAL_HALF_PERIOD) or 2 pi; velocity difference; 1 -
 *             [attribute equal], NaN when the ground truth has none.  An error the class does not define (flags) is NaN.
 *  records    32 bytes per detection row at slot (cursor + b) M + row of `records`: fp32 score; a word with the class in
 *             bits 0-7, valid in bit 8 and the thresholds' true-positive bits in 16-19; the five fp32 errors (trans,
 *             scale, orient, vel, attr; NaN without a match at dist_th_tp); one zero word.  Every slot of the batch is
 *             written once, rows at or beyond counts[b] and filtered rows as invalid (all zero).
 *  state      int64: [0] the sample cursor (read here; the caller adds B on the same stream afterwards), [1] samples
 *             with counts[b] > max_boxes_per_sample, [2] (sample, class) pairs with more than VAMP_DET_EVAL_GT_CAP
 *             ground-truth boxes, [3] labels outside [0, num_classes) (padding excepted), [4] batches that did not fit
 *             (cursor + B > max_samples: nothing else is written), [8 + c] the surviving ground truth of class c.
 *             All by integer atomic adds.
 * Limits: 1 <= B <= 4096, 1 <= M <= VAMP_DET_EVAL_MAX_WIDTH, 0 <= G <= 2^20, box_cols 7 | 9, 1 <= num_classes <=
 * VAMP_DET_EVAL_MAX_CLASSES, ascending positive thresholds with dist_th_tp among them, max_samples M < 2^31.  Every
 * argument is checked before any device work.  One launch on `stream`, one workgroup per (sample, class); no float
 * atomics, no host synchronisation, the record bytes are a pure function of the inputs; capturable in a graph.
 * -------------------------------------------------------------------------- */
#define VAMP_DET_EVAL_MAX_CLASSES 16
#define VAMP_DET_EVAL_GT_CAP 256        /* ground-truth boxes of one class in one sample held in LDS */
#define VAMP_DET_EVAL_MAX_WIDTH 2048
#define VAMP_DET_EVAL_RECORD_BYTES 32
#define VAMP_DET_EVAL_STATE_WORDS 24    /* int64 words of `state`: 8 counters, then VAMP_DET_EVAL_MAX_CLASSES npos */
enum { VAMP_DET_EVAL_HALF_PERIOD = 1, VAMP_DET_EVAL_HAS_ORIENT = 2, VAMP_DET_EVAL_HAS_VEL = 4, VAMP_DET_EVAL_HAS_ATTR = 8 };
typedef struct VampDetEvalDesc {
  double class_range[VAMP_DET_EVAL_MAX_CLASSES];   /* metres */
  double dist_ths[4];                              /* ascending */
  double dist_th_tp;                               /* one of dist_ths */
  int32_t B, M, G;
  int32_t box_cols;                                /* 7 | 9 */
  int32_t score_dtype;                             /* VAMP_F32 | VAMP_BF16 | VAMP_F16 */
  int32_t gt_label_dtype;                          /* VAMP_I32 | VAMP_I64 */
  int32_t has_attrs;                               /* 0 | 1 */
  int32_t num_classes;
  int32_t max_boxes_per_sample;
  int32_t max_samples;                             /* capacity of `records` in samples */
  int32_t class_flags[VAMP_DET_EVAL_MAX_CLASSES];  /* VAMP_DET_EVAL_* bits */
  int32_t attr_moving[VAMP_DET_EVAL_MAX_CLASSES];  /* predicted attribute above 0.2 m/s, -1: none */
  int32_t attr_still[VAMP_DET_EVAL_MAX_CLASSES];   /* ... and at or below */
  int32_t reserved[2];                             /* 0 */
} VampDetEvalDesc;
int vamp_det_eval_supported(const VampDetEvalDesc* d);
size_t vamp_det_eval_record_bytes(const VampDetEvalDesc* d);
int vamp_det_eval_update(const VampDetEvalDesc* d, const float* boxes, const void* scores, const int32_t* labels,
                         const int32_t* counts, const float* gt_boxes, const void* gt_labels, const int8_t* gt_attrs,
                         void* records, int64_t* state, void* stream);

/* --------------------------------------------------------------------------
 * Batch normalisation of an [N, C, H, W] NCHW-contiguous tensor with the ReLU and the residual add that follow it in
 * the encoders, synchronised over `world` ranks (base_cli.py:78, 91 Trainer(sync_batchnorm=True): Lightning turns every
 * BatchNorm2d of the model into a synchronised one).  Four steps, so that the caller's collective can sit between
 * the first and the second of each direction; world = 1 is the plain single-GPU norm.  x, residual, y, dy, dx and
 * grad_residual share one element type (dtype: VAMP_F32 | VAMP_BF16 | VAMP_F16) and must be 16-byte aligned; weight,
 * bias, the running statistics, saved and the gradients of weight and bias are fp32; the rows are float64.
 *
 *  partial_stats     row [2 C + 1] of THIS rank: n = N H W, then per channel mean and M2 = sum (x - mean)^2, float64,
 *                    per workgroup over VAMP_BN_CHUNK elements of a channel (sums of x - first element, so nothing
 *                    cancels), the chunks merged in index order by Chan's formula.
 *  apply             rows [world, 2 C + 1] in rank order, merged per channel in rank order by Chan's formula
 *                    (n = na + nb, delta = mb - ma, mean = ma + delta nb / n, M2 = M2a + M2b + delta^2 na nb / n);
 *                    var = M2 / n, invstd = 1 / sqrt(var + eps).  y = act(weight (x - mean) invstd + bias [+ residual])
 *                    in fp32, rounded once to dtype; act is ReLU (a NaN stays a NaN) or none.  saved [3, C] fp32
 *                    receives mean, invstd and the low word of the float64 mean (mean = saved[0] + saved[2]), which
 *                    the backward takes.  update_running: running_mean = (1 - momentum) running_mean + momentum mean,
 *                    running_var = (1 - momentum) running_var + momentum var n / (n - 1) with the global n, one
 *                    workgroup per channel writing them; num_batches_tracked (int64, may be NULL) is incremented.
 *                    training = 0 (evaluation): mean and 1 / sqrt(running_var + eps) come from the running statistics,
 *                    rows is not read, nothing is updated, saved may be NULL.
 *  backward_partial  dz = dy where y > 0 (or y is NaN), else 0, under ReLU -- y the saved output, there is no mask --
 *                    else dz = dy.  row [2 C] of this rank: per channel sum dz and sum dz (x - mean), float64, fixed
 *                    order; grad_bias = sum dz and grad_weight = invstd sum dz (x - mean) of this rank in fp32.
 *  backward_apply    rows [world, 2 C] added in rank order, the global n from stat_rows (the forward's rows);
 *                    dx = weight invstd (dz - sum dz / n - (x - mean) invstd^2 sum dz (x - mean) / n),
 *                    grad_residual = dz (has_residual), each rounded once to dtype, every element written once.
 * Launches at world = 1: two per direction when N H W <= VAMP_BN_CHUNK (one workgroup per channel), else three (the
 * chunks' partials are merged by a launch of their own).  No atomics, no host synchronisation, bitwise repeatable,
 * capturable in a graph.  The workspace (8-byte aligned, vamp_bn_workspace_bytes: 24 bytes per channel and chunk)
 * needs no initialisation and is free again after each call.
 * Limits, checked before any launch (VAMP_EINVAL with a message, and a workspace size of 0): C >= 1, N, H, W >= 1,
 * N H W < 2^31, C ceil(N H W / VAMP_BN_CHUNK) < 2^31, 1 <= world <= VAMP_BN_MAX_WORLD, a known dtype and act,
 * has_residual with its pointer, float64 rows 8-byte aligned; a workspace that is NULL or too small VAMP_ENOSPC.
 * -------------------------------------------------------------------------- */
#define VAMP_BN_CHUNK 4096        /* elements of one channel per workgroup */
#define VAMP_BN_MAX_WORLD 64
enum { VAMP_BN_ACT_NONE = 0, VAMP_BN_ACT_RELU = 1 };
typedef struct VampBatchNormDesc {
  double eps, momentum;
  int32_t N, C, H, W;
  int32_t dtype;                  /* VAMP_F32 | VAMP_BF16 | VAMP_F16 */
  int32_t act;                    /* VAMP_BN_ACT_* */
  int32_t has_residual;           /* 0 | 1 */
  int32_t training;               /* 0: evaluation (running statistics) | 1 */
  int32_t world;                  /* ranks whose rows are merged, 1 .. VAMP_BN_MAX_WORLD */
  int32_t update_running;         /* 0 | 1: apply updates the running statistics (training only) */
  int32_t reserved[2];            /* 0 */
} VampBatchNormDesc;
size_t vamp_bn_workspace_bytes(const VampBatchNormDesc* d);
int vamp_bn_partial_stats(const VampBatchNormDesc* d, const void* x, double* row, void* workspace,
                          size_t workspace_bytes, void* stream);
int vamp_bn_apply(const VampBatchNormDesc* d, const void* x, const void* residual, const double* rows,
                  const float* weight, const float* bias, float* running_mean, float* running_var,
                  int64_t* num_batches_tracked, void* y, float* saved, void* stream);
int vamp_bn_backward_partial(const VampBatchNormDesc* d, const void* dy, const void* x, const void* y,
                             const float* saved, double* row, float* grad_weight, float* grad_bias, void* workspace,
                             size_t workspace_bytes, void* stream);
int vamp_bn_backward_apply(const VampBatchNormDesc* d, const void* dy, const void* x, const void* y,
                           const float* saved, const float* weight, const double* rows, const double* stat_rows,
                           void* dx, void* grad_residual, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VAMPIRE_HIP_H_ */
