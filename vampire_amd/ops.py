"""Host-side operators of the lift + render hot path (Python over the C ABI).

`HotPath` owns the per-configuration device constants (axis arrays, descriptors)
and exposes the operators with autograd support:

  lift(depth, feat, lift_mats)                       ~ bv2:550-553 + get_voxel_feats
  lift_dense(frustum_feats, lift_mats)               ~ get_voxel_feats signature (bv2:483)
  render(geom|render_mats, density_feature, semantic_logits, base, rgb, beta)
                                                     ~ volume_rendering_from_multiple_views (bv2:391)

All heavy work happens in hand-written HIP kernels reached through ctypes
(`_capi`); torch supplies device memory and the current stream only.
"""
import ctypes as C
import math
import os

import torch

from . import _capi
from .config import PathConfig
from . import geometry as G
from ._tensors import (_accept, _accept_float, _chk, _density_code, _dtype_code, _is_channel_last, _mats, _scalar,
                       _stream, need_device)
# the operators that take no HotPath live in modules of their own; their public names stay importable from here
from .layers import (voxel_pooling, upsample_trilinear, conv3d_3x3x3, conv3d_bf16, conv3d_supported,  # noqa: F401
                     conv3d_bf16_supported, conv3d_bf16_stride2, conv3d_bf16_stride2_supported,
                     resize_bilinear2d, resize_bilinear2d_pack, resize_bilinear2d_supported,
                     HeadSegment, conv3d_fused, conv3d_heads)
from .evaluation import (confusion_update, lidarseg_predict, det_postprocess, det_targets, det_loss,  # noqa: F401
                         DetResult, DetTargets)
from .losses import REG_MAX_TERMS, REG_TILE, RegTerm, reg_loss, reg_losses, rgb_loss, seg_loss  # noqa: F401


# det-grid heights the BEV kernels take: their z taps and weights live in fixed LDS tables (kBevMaxOZ, render_bev_dev.hpp)
BEV_MAX_OZ = 64


def lift_desc(cfg: PathConfig, B, N, C_, dtype_code, use_depth=True, fhw=None) -> _capi.VampLiftDesc:
    """The lift descriptor of `cfg` for B samples of N cameras with C_ feature channels; host only, no device needed.
    `fhw`: size of the image feature map when it is not final_dim / downsample_factor -- the lift
    samples it in normalised coordinates (bv2:499-507), so any resolution works: the reference's own
    ResNet-50 + SECONDFPN(upsample_strides=[0.5, 1, 2, 4]) delivers stride-8 maps (32 x 88) beside
    the stride-4 frustum of the renderer."""
    c = cfg
    d = _capi.VampLiftDesc()
    d.B, d.N, d.C = B, N, C_
    d.D = c.D if use_depth else 1
    d.fH, d.fW = (c.fH, c.fW) if fhw is None else (int(fhw[0]), int(fhw[1]))
    d.Z, d.Y, d.X = c.vZ, c.vY, c.vX
    d.u_max, d.v_max = float(c.final_dim[1] - 0.5), float(c.final_dim[0] - 0.5)
    d.u_div, d.v_div = float(c.final_dim[1] - 1), float(c.final_dim[0] - 1)
    d.d_lo, d.d_hi = c.d_bound[0], c.d_bound[1]
    d.d_span = c.d_bound[1] - c.d_bound[0]          # python double -> fp32, as torch does
    d.use_depth = 1 if use_depth else 0
    d.in_dtype = dtype_code
    return d


def render_desc(cfg: PathConfig, B, N, dtype_code, C_=None) -> _capi.VampRenderDesc:
    """The render descriptor of `cfg` for B samples of N cameras (C_: mid channels, default cfg.mid_channels); host
    only, no device needed."""
    c = cfg
    d = _capi.VampRenderDesc()
    d.B, d.N = B, N
    d.D, d.fH, d.fW = c.D, c.fH, c.fW
    d.K, d.C = c.num_classes, (c.mid_channels if C_ is None else C_)
    d.Z, d.Y, d.X = c.vZ, c.vY, c.vX
    d.oZ, d.oY, d.oX = c.oZ, c.oY, c.oX
    bounds = (c.x_bound_seg, c.y_bound_seg, c.z_bound_seg)
    for i, b in enumerate(bounds):
        d.lo[i] = b[0]
        d.span[i] = b[1] - b[0]
    d.d_far = c.d_bound[1]
    d.z_step_det = c.z_bound_det[2]
    for i, bnd in enumerate((c.x_bound_det, c.y_bound_det, c.z_bound_det)):
        d.det_step[i] = bnd[2]
    d.density_mode = _density_code(c)
    d.sdf_bias = c.sdf_bias
    d.beta_min = 1e-4
    d.cat_seg = 1 if c.cat_seg else 0
    d.in_dtype = dtype_code
    return d


class CounterState:
    """Which cell counters of the lift and render workspaces are known to be zero; host only, no device needed.

    The counters (`cnt`) lie behind regions whose sizes follow the descriptor (lift_common.hpp, render_common.hpp), so
    "known zero" is a fact about (workspace key, buffer address, the (offset, bytes) of `cnt` for one descriptor), never
    about the key alone: a call of another descriptor on the same buffer zeroes other bytes, and its own regions may lie
    over these.  Per key the state is one (address, range) pair, range None standing for every range of a buffer that
    has been zero-filled and not used since; no entry = nothing known.  A *_CLEAN promise is sent only on `begin`
    returning True; without it the library zero-fills."""

    def __init__(self):
        self._zero = {}

    def fresh(self, key, addr):
        """A new zero-filled buffer: every range is clean until the first call on it."""
        self._zero[key] = (addr, None)

    def use(self, key, addr, rng):
        """A call of the layout whose counters are `rng` is about to work on the buffer.  No region of a layout
        overlaps that layout's own counters (but for the v1 camera splat's gradient copy: its backward calls `spoil`),
        so they stay what they were; what was known of any other range is void."""
        z = self._zero.get(key)
        if z is not None and z[0] == addr and z[1] in (None, rng):
            self._zero[key] = (addr, rng)
        else:
            self._zero.pop(key, None)

    def begin(self, key, addr, rng):
        """A pass that counts into `rng` starts: True if the range is known zero.  From here the counters are in
        flight -- not clean -- until `done`; a call that raises in between leaves them so."""
        z = self._zero.pop(key, None)
        return z is not None and z[0] == addr and z[1] in (None, rng)

    def done(self, key, addr, rng):
        """The pass over `rng` has been issued in full (its scan zeroes what it reads): clean for this range and for
        no other.  (A pass that ends on a buffer the key no longer names -- a larger one has replaced it since -- says
        nothing about the new one.)"""
        z = self._zero.get(key)
        if z is None or z[0] == addr:
            self._zero[key] = (addr, rng)

    def spoil(self, key):
        """Something may have left any counters of the buffer non-zero."""
        self._zero.pop(key, None)


class HotPath:
    """Device constants + operators for one PathConfig on one device."""

    def __init__(self, cfg: PathConfig, device="cuda"):
        if cfg.oZ > BEV_MAX_OZ:
            # (refused here, before any device work: the library would refuse every BEV call)
            raise ValueError(f"z_bound_det gives {cfg.oZ} heights: the BEV kernels take at most {BEV_MAX_OZ} "
                             "det-grid heights")
        self.cfg = cfg
        self.device = torch.device(device)
        self.lib = _capi.load()     # (sets self.vamp too: the `lib` property below)
        geo = G.PathGeometry(cfg)
        dev = self.device
        f32 = torch.float32
        # axis arrays (the kernels rebuild points from these; bit-identical to the buffers)
        self.xs = G.axis_centres(cfg.x_bound_seg).to(dev)
        self.ys = G.axis_centres(cfg.y_bound_seg).to(dev)
        self.zs = G.axis_centres(cfg.z_bound_seg).to(dev)
        self.oxs = G.axis_centres(cfg.x_bound_det).to(dev)
        self.oys = G.axis_centres(cfg.y_bound_det).to(dev)
        self.ozs = G.axis_centres(cfg.z_bound_det).to(dev)
        self.us = geo.frustum[0, 0, :, 0].contiguous().to(dev)
        self.vs = geo.frustum[0, :, 0, 1].contiguous().to(dev)
        self.ds = geo.frustum[:, 0, 0, 2].contiguous().to(dev)
        self.camera_mids = geo.camera_mids.to(dev)
        self.bev_mids = geo.bev_mids.to(dev)
        ozs_cpu = G.axis_centres(cfg.z_bound_det)
        self.ozs_host = (C.c_float * ozs_cpu.numel())(*ozs_cpu.tolist())
        self._ws = {}
        # state of the camera-forward choice ("auto"): mode, call counter, the statistic on the device / in pinned memory
        self._cam_sel = {"mode": "direct", "calls": 0,
                         "dev": torch.full((1,), -1.0, dtype=f32, device=dev),
                         "host": torch.full((1,), -1.0, dtype=f32).pin_memory() if dev.type == "cuda" else torch.full((1,), -1.0)}
        self._counters = CounterState()     # which cell counters of the "lift" / "render" workspaces are known zero
        self._cnt_ranges = {}               # (key, descriptor bytes) -> (offset, bytes) of that layout's counters
        # Implementation selectors (host-side state of this object; the library itself keeps none):
        # "cell" = the default cell-list gathers, "v1" = the float-atomic splats kept as independent
        # cross-checks for the tests; lift_wpp forces the lift gather's waves per pixel (0 = auto).
        # The environment gives the initial values only.
        self.impl = {"cam_bwd": os.environ.get("VAMP_CAM_BWD", "cell"),
                     # lift backward: "cell" = cell list + gather (default), "v1" = float-atomic splat
                     "lift_bwd": os.environ.get("VAMP_LIFT_BWD", "cell"),
                     "bev_bwd": os.environ.get("VAMP_BEV_BWD", "cell"),
                     "lift_wpp": int(os.environ.get("VAMP_LIFT_WPP", "0")),
                     # BEV branch on a second stream in training steps (forward-only calls stay on one
                     # stream): eager step 0.679 vs 0.699 ms, replayed from a HIP graph 0.629 vs 0.695 ms
                     "overlap": os.environ.get("VAMP_OVERLAP", "1") == "1",
                     # early ray termination in the camera branch (include/vampire_hip.h)
                     "ert": os.environ.get("VAMP_ERT", "1") != "0",
                     # the camera branch as ONE kernel on the channel-first volumes (no packed copy, no
                     # separate termination pass; render_cam_direct.hip), or the channel-last copy + planned march.
                     # The one kernel wins where rays saturate early (48 against 19 + 26 + ... us) and loses where they
                     # do not (cfg-B: 185 - 222 us against 26 + 126: 64 far-field rays of a wave touch 64 lines per pair
                     # load of a channel-first volume).  "auto" (default): chosen per call from the termination tables
                     # of the last calls (_camera_forward_choice); True / False force one
                     "cam_direct": {"1": True, "0": False}.get(os.environ.get("VAMP_CAM_DIRECT", "auto"), "auto"),
                     # the render forward's two branches as ONE launch (render_fwd_merged.hip: camera tiles first, BEV
                     # column blocks filling the slots the camera tiles' tail leaves idle) wherever the one-kernel camera
                     # forward with early termination runs; False = the two launches (the tests' cross-check: same bits)
                     "fwd_merged": True,
                     # the BEV forward as one kernel (render_bev_fused.hip); False = the two-kernel first
                     # implementation, the cross-check of the tests
                     "bev_fused": True,
                     # forward-only calls: BEV branch on the side stream beside the camera branch.  Off for
                     # eager launches (the fork / join costs more than it hides); a caller that captures the
                     # forward into a HIP graph switches it on (bench.py)
                     "fwd_overlap": False,
                     # training: the camera forward keeps every inside sample's values for the backward's per-ray pass
                     # (+0.5 GB of workspace per sample at cfg-B, touched only where samples are kept); False = that pass
                     # gathers again (the tests' cross-check of the re-sampling path; no environment switch)
                     "save_rows": True,
                     # a training lift forward leaves the scan of its pair cells to the render forward's prepare step,
                     # which scans both operators' cell lists in ONE launch (vamp_render_camera_prepare_with_lift); a lift
                     # backward, or another lift forward, that finds the scan still pending runs it itself
                     # (vamp_lift_finish_cells).  False = the scan inside the lift forward's call (no environment switch)
                     "defer_lift_scan": True}
        self._lift_scan_pending = None      # (desc, workspace, stream) of a lift forward whose cell scan is still due
        # What the workspaces hold, as generation counters (a forward keeps (counter, buffer address) and its backward
        # compares) -- each with what makes an earlier forward's leavings stale:
        self._lift_gen = 0          # lift pair cells: any later lift forward or lift backward
        self._bev_gen = 0           # BEV forward's samples: any later BEV forward (alone or inside the merged launch)
        self._pack_gen = 0          # render workspace: any later render forward, render backward or ert_statistics
        self._bev_tab_key = None    # (BEV workspace address, B) of a split BEV backward's axis tables: a new buffer or B
        self._side = None           # the side stream, made on first use: a caller resets it to None to get a fresh one

    # ------------------------------------------------------------- the library
    # `lib` hands status codes back as integers; `vamp` is the same entry points raising VampireHipError on a failure,
    # which every call of this file goes through.  Assigning `lib` (a test's call recorder around the library) re-derives
    # `vamp`, so that the calls still pass through whatever `lib` is.
    @property
    def lib(self):
        return self._lib

    @lib.setter
    def lib(self, lib):
        self._lib, self.vamp = lib, _capi.checked(lib)

    # ---------------------------------------------------------------- descs
    def lift_desc(self, B, N, C_, dtype_code, use_depth=True, fhw=None) -> _capi.VampLiftDesc:
        return lift_desc(self.cfg, B, N, C_, dtype_code, use_depth, fhw)

    def render_desc(self, B, N, dtype_code, C_=None) -> _capi.VampRenderDesc:
        return render_desc(self.cfg, B, N, dtype_code, C_)

    def _side_stream(self):
        """Second HIP stream for the BEV branch of the renderer: it shares no kernel with the camera
        branch, and at batch 1 neither fills the 256 CUs alone (VAMP_OVERLAP=0 disables)."""
        if not self.impl["overlap"]:
            return None
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        return self._side

    def _finish_lift_scan(self):
        """Run the cell scan a training lift forward deferred (impl["defer_lift_scan"]), if it is still due."""
        p, self._lift_scan_pending = self._lift_scan_pending, None
        if p is None:
            return
        d, ws, st = p
        cur = torch.cuda.current_stream()
        if cur != st:
            cur.wait_stream(st)
        self.vamp.vamp_lift_finish_cells(d, ws, ws.numel(), _stream(cur))
        self._counters.done("lift", ws.data_ptr(), self._cnt_range("lift", d))      # scanned: back at zero

    def _cnt_range(self, key, d):
        """(offset, bytes) of the cell counters in the "lift" / "render" workspace of descriptor `d`, from the library's
        own layout; asked once per descriptor."""
        k = (key, bytes(d))
        r = self._cnt_ranges.get(k)
        if r is None:
            ask = _capi.checked()           # (a host-only query: not through a test's call recorder)
            if key == "lift":
                lay, i = _capi.VampLiftWorkspaceLayout(), _capi.LIFTWS_REGIONS.index("cnt")
                ask.vamp_lift_workspace_layout(d, lay)
            else:
                lay, i = _capi.VampRenderWorkspaceLayout(), _capi.RENDERWS_REGIONS.index("cnt")
                ask.vamp_render_workspace_layout(d, lay)
            r = self._cnt_ranges[k] = (int(lay.offset[i]), int(lay.bytes[i]))
        return r

    def _cam_clean_flag(self, d, ws):
        """VAMP_CAMPREP_COUNTERS_CLEAN when the cell counters of descriptor `d` in the render workspace `ws` are known
        to be zero (fresh zero-filled buffer, or the last pass on it was one of this layout and was issued in full);
        marks them in flight."""
        clean = self._counters.begin("render", ws.data_ptr(), self._cnt_range("render", d))
        return _capi.VAMP_CAMPREP_COUNTERS_CLEAN if clean else 0

    # ------------------------------------------------- which camera forward (bv2:191-194: both density modes are first class)
    # Two candidates when early termination is allowed: the ONE KERNEL with termination, whose cost follows the
    # samples the rays keep, and the channel-last COPY + PLANNED MARCH of every inside sample without it (the
    # termination pre-pass of the planned march never pays: where rays saturate the one kernel is faster, where
    # they do not the pre-pass marches every sample itself -- cfg-B, sigmoid density: forward 291 us with it, 230
    # without, 257 for the one kernel; training step 899 / 878 / 979).
    # The statistic: mean over the 8 x 8 ray tiles of (largest number of leading samples a ray of the tile keeps)
    # / (samples per ray) -- what the one kernel's cost follows -- from the termination table in the workspace
    # (0.09 on the synthetic sdf workload, 0.69 under the sigmoid density; the two forwards cost the same near
    # 0.5 - 0.6).
    # DETERMINISTIC (round 6): the statistic is formed on the device at fixed call indices (every _PROBE_EVERY-th
    # eager call), copied to pinned host memory behind an event, and APPLIED at a fixed later call index
    # (_PROBE_LAG calls on), where the host waits for that event -- long done by then, so the wait costs nothing.
    # Which call switches is therefore a function of the call index and the data alone: two runs of one seed (and
    # the ranks of a data-parallel job on equal data) take the same kernels in every call.  (Round 5 read the
    # pinned word whenever it happened to have landed: the switch depended on host timing.)
    _PROBE_EVERY = 16            # one-kernel mode: the table is the forward's by-product; the probe is two small reductions
    _PROBE_EVERY_PLANNED = 64    # planned mode leaves no table: the density-only pre-pass (20 - 60 us) is run for the probe
    _PROBE_LAG = 8               # calls between a probe and the call that applies it
    _TO_PLANNED, _TO_DIRECT = 0.5, 0.4                           # hysteresis

    def camera_forward_mode(self):
        """The camera forward the next "auto" call takes ("direct" = one kernel + early termination, "planned" = copy +
        planned march), for logs: bench.py reports it beside the captured step."""
        return self._cam_sel["mode"]

    def _camera_forward_choice(self, can_direct, no_geom):
        """(ert, direct) of this call."""
        ert_allowed = no_geom and self.impl["ert"]
        sel = self.impl["cam_direct"]
        if sel != "auto" or not ert_allowed or not can_direct:
            want = ert_allowed if sel == "auto" else bool(sel)
            return ert_allowed, bool(can_direct and want)
        st = self._cam_sel
        pend = st.get("pending")
        # a probe is applied at ITS call index + lag, never earlier or later (calls under graph capture do not count:
        # a captured graph keeps the variant of its capture)
        if pend is not None and st["calls"] + 1 >= pend[0] and not torch.cuda.is_current_stream_capturing():
            pend[1].synchronize()
            r = float(st["host"][0])
            st["last"] = r
            st["pending"] = None
            if st["mode"] == "direct" and r > self._TO_PLANNED:
                st["mode"] = "planned"
            elif st["mode"] == "planned" and r < self._TO_DIRECT:
                st["mode"] = "direct"
        return (True, True) if st["mode"] == "direct" else (False, False)

    def _camera_forward_probe(self, d, ws, tensors, ert, no_geom, stream):
        """The eager calls of the auto mode at the probe indices: the statistic of this call's termination table."""
        if self.impl["cam_direct"] != "auto" or not (no_geom and self.impl["ert"]):
            return
        if torch.cuda.is_current_stream_capturing():
            return
        st = self._cam_sel
        st["calls"] += 1
        every = self._PROBE_EVERY if ert else max(self._PROBE_EVERY, self._PROBE_EVERY_PLANNED if self._PROBE_EVERY > 1 else 1)
        if (st["calls"] - 1) % every or st.get("pending") is not None:
            return
        c = self.cfg
        if not ert:
            mats, beta, dens = tensors
            self.vamp.vamp_render_camera_terminate(d, mats, self.us, self.vs, self.ds, beta, dens, ws, ws.numel(),
                                                  _stream(stream))
        term = self._term_table(d, ws).view(d.B * d.N, 1, c.fH, c.fW)
        tile_max = torch.nn.functional.max_pool2d(term.float(), 8, ceil_mode=True)
        st["dev"].copy_((tile_max.mean() / float(c.D - 1)).reshape(1))
        st["host"].copy_(st["dev"], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        st["pending"] = [st["calls"] + min(self._PROBE_LAG, every - 1 if every > 1 else 1), ev]

    def _workspace(self, key, nbytes):
        t = self._ws.get(key)
        if t is None or t.numel() < nbytes:
            # zero-filled once: the cell counters inside start clean, and every completed pass leaves its own layout's
            # clean again (VAMP_LIFTFWD_CELLS_CLEAN / VAMP_CAMPREP_COUNTERS_CLEAN), so no steady-state step zeroes them
            t = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=self.device)
            self._ws[key] = t
            self._counters.fresh(key, t.data_ptr())
        return t

    def _render_workspace(self, d, rows=False):
        """The render workspace of a call on descriptor `d`: with room for the kept sample rows behind it, or without."""
        nbytes = self.vamp.vamp_render_workspace_bytes(d)
        if rows:
            nbytes += self.vamp.vamp_render_samples_bytes(d)
        ws = self._workspace("render", nbytes)
        self._counters.use("render", ws.data_ptr(), self._cnt_range("render", d))
        return ws

    def _lift_workspace(self, d):
        """The lift workspace of a call on descriptor `d`."""
        ws = self._workspace("lift", self.vamp.vamp_lift_workspace_bytes(d))
        self._counters.use("lift", ws.data_ptr(), self._cnt_range("lift", d))
        return ws

    def _term_table(self, d, ws):
        """The termination table inside the render workspace `ws`: a flat int32 view, one entry per ray."""
        off = self.vamp.vamp_render_term_offset(d)
        return ws[off:off + 4 * d.B * d.N * d.fH * d.fW].view(torch.int32)

    # ----------------------------------------------------------------- lift
    def lift(self, depth, feat, lift_mats, use_depth=True):
        """depth [B,N,D,fH,fW], feat [B,N,C,fH,fW], lift_mats [B,N,3,4,4] -> [B,C,Z,Y,X]."""
        with torch.cuda.device(self.device):      # launches go to this object's device, whatever is current
            return _LiftFn.apply(self, depth, feat, lift_mats, use_depth, torch.is_grad_enabled())

    def lift_logits(self, logits, feat, lift_mats):
        """The lift fed with the raw depth LOGITS [B,N,D,fH,fW] (fp32 | bf16): the softmax of bv2:550 runs
        in the launch that prepares the lift's operands and its backward inside the lift backward's
        gather (producer side) -- same values as ``lift(logits.softmax(2), feat, mats)``."""
        with torch.cuda.device(self.device):
            return _LiftFn.apply(self, logits, feat, lift_mats, True, torch.is_grad_enabled(), True)

    def lift_dense(self, frustum_feats, lift_mats):
        """frustum_feats [B,N,C,D,fH,fW] (materialised, fp32) -> [B,C,Z,Y,X]."""
        return _LiftDenseFn.apply(self, frustum_feats, lift_mats)

    def lift_indices(self, lift_mats, use_depth=True):
        c = self.cfg
        B, N = lift_mats.shape[:2]
        d = self.lift_desc(B, N, 4, _capi.VAMP_F32, use_depth)
        shp = (B, N, c.vZ, c.vY, c.vX)
        valid = torch.empty(shp, dtype=torch.uint8, device=self.device)
        ix0, iy0, iz0 = (torch.empty(shp, dtype=torch.int16, device=self.device) for _ in range(3))
        mats = _mats(lift_mats, B, N, "lift_mats")
        self.vamp.vamp_lift_indices(d, mats, self.xs, self.ys, self.zs, valid, ix0, iy0, iz0, _stream())
        return valid, ix0, iy0, iz0

    def lift_cull_words(self, lift_mats, use_depth=True):
        """The forward's camera cull words [B, Z, grid_y, grid_x] (uint32 as int64) and the patch shape
        (px, py) in voxels: bit n clear = no voxel of the patch can be valid in camera n (diagnostic)."""
        c = self.cfg
        B, N = lift_mats.shape[:2]
        d = self.lift_desc(B, N, 4, _capi.VAMP_F32, use_depth)
        patch, grid = (C.c_int32 * 2)(), (C.c_int32 * 2)()
        mats = _mats(lift_mats, B, N, "lift_mats")
        self.vamp.vamp_lift_cull_words(d, None, None, None, None, None, patch, grid, None)
        words = torch.empty(B, c.vZ, grid[1], grid[0], dtype=torch.int32, device=self.device)
        self.vamp.vamp_lift_cull_words(d, mats, self.xs, self.ys, self.zs, words, patch, grid, _stream())
        return words.long() & 0xffffffff, (patch[0], patch[1])

    # --------------------------------------------------------------- render
    def frustum_geometry(self, render_mats):
        c = self.cfg
        B, N = render_mats.shape[:2]
        d = self.render_desc(B, N, _capi.VAMP_F32)
        mats = _chk(render_mats.float(), (B, N, 3, 4, 4), "render_mats")
        geom = torch.empty(B, N, c.D, c.fH, c.fW, 3, dtype=torch.float32, device=self.device)
        self.vamp.vamp_frustum_geometry(d, mats, self.us, self.vs, self.ds, geom, _stream())
        return geom

    def render_indices(self, geom=None, render_mats=None):
        c = self.cfg
        src = geom if geom is not None else render_mats
        B, N = src.shape[:2]
        d = self.render_desc(B, N, _capi.VAMP_F32)
        shp = (B, N, c.D - 1, c.fH, c.fW)
        inside = torch.empty(shp, dtype=torch.uint8, device=self.device)
        ix0, iy0, iz0 = (torch.empty(shp, dtype=torch.int16, device=self.device) for _ in range(3))
        g = None if geom is None else _chk(geom.float(), (B, N, c.D, c.fH, c.fW, 3), "geom")
        m = None if render_mats is None else _chk(render_mats.float(), (B, N, 3, 4, 4), "render_mats")
        self.vamp.vamp_render_indices(d, g, m, self.us, self.vs, self.ds, inside, ix0, iy0, iz0, _stream())
        return inside, ix0, iy0, iz0

    def render_direct_taps(self, render_mats, coords=False):
        """Diagnostics: (inside, ix0, iy0, iz0[, fxyz]) of every ray sample as the one-kernel camera forward
        evaluates them (vamp_render_camera_direct_taps)."""
        c = self.cfg
        B, N = render_mats.shape[:2]
        d = self.render_desc(B, N, _capi.VAMP_F32)
        shp = (B, N, c.D - 1, c.fH, c.fW)
        inside = torch.empty(shp, dtype=torch.uint8, device=self.device)
        ix0, iy0, iz0 = (torch.empty(shp, dtype=torch.int16, device=self.device) for _ in range(3))
        fxyz = torch.empty(shp + (3,), dtype=torch.float32, device=self.device) if coords else None
        m = _chk(render_mats.float(), (B, N, 3, 4, 4), "render_mats")
        self.vamp.vamp_render_camera_direct_taps(d, m, self.us, self.vs, self.ds, inside, ix0, iy0, iz0, fxyz, _stream())
        return (inside, ix0, iy0, iz0) + ((fxyz,) if coords else ())

    def render(self, density_feature, semantic_logits, base, rgb, beta=None, *, geom=None,
               render_mats=None):
        """The reference's 8-tuple (bv2:462-467).  Give either ``geom`` [B,N,D,fH,fW,3]
        (API-compatible) or ``render_mats`` [B,N,3,4,4] (geometry evaluated in-kernel)."""
        if (geom is None) == (render_mats is None):
            raise ValueError("give exactly one of geom / render_mats")
        if beta is None:
            beta = torch.zeros((), device=self.device)
            if self.cfg.density_mode == "sdf":
                raise ValueError("density_mode='sdf' needs the beta parameter")
        with torch.cuda.device(self.device):
            return _RenderFn.apply(self, density_feature, semantic_logits, base, rgb, beta, geom,
                                   render_mats, torch.is_grad_enabled())

    def ert_statistics(self, density_feature, beta, render_mats):
        """What early ray termination removes on these inputs: (inside samples, inside samples the
        per-ray table keeps).  Diagnostic for bench.py (the gain is data-dependent); one termination
        pre-pass + the index kernel, a host sync."""
        c = self.cfg
        B, N = render_mats.shape[:2]
        dens = _chk(_accept_float(density_feature, "density_feature"), (B, 1, c.vZ, c.vY, c.vX), "density_feature")
        d = self.render_desc(B, N, _dtype_code(dens))
        mats = _chk(render_mats.float(), (B, N, 3, 4, 4), "render_mats")
        beta = torch.zeros(1, device=self.device) if beta is None else _scalar(beta.detach(), "beta")
        ws = self._render_workspace(d)
        with torch.cuda.device(self.device):
            self.vamp.vamp_render_camera_terminate(d, mats, self.us, self.vs, self.ds, beta, dens, ws, ws.numel(),
                                                  _stream())
            term = self._term_table(d, ws).reshape(B, N, 1, c.fH, c.fW).clone()
            inside = self.render_indices(render_mats=mats)[0].bool()
        idx = torch.arange(c.D - 1, device=self.device).reshape(1, 1, -1, 1, 1)
        self._pack_gen += 1         # the workspace no longer matches a saved forward
        return int(inside.sum()), int((inside & (idx < term)).sum())

    # ------------------------------------------------------ point resampling
    def sample_points(self, volume, points, *, padding="zeros", mask_outside=False, activation=False,
                      beta=None, channel_last=False, lattice=None):
        """F.grid_sample(volume, normalised points, padding_mode=padding, align_corners=True) as the
        reference uses it for the occupancy and lidar-point queries (bv2:576-609).

        volume [B,C,Z,Y,X]; points [B,P,3] ego-frame xyz (normalised by the seg bounds inside);
        returns [B,C,P] (or [B,P,C] with channel_last).  ``activation`` samples density(volume)
        (occ_density, bv2:604); ``mask_outside`` multiplies by all(-1 <= n <= 1) (pts_sdf, bv2:595)."""
        if beta is None:
            beta = torch.zeros((), device=self.device)
            if activation and self.cfg.density_mode == "sdf":
                raise ValueError("density_mode='sdf' needs the beta parameter")
        return _SamplePointsFn.apply(self, volume, points, beta, padding, bool(mask_outside),
                                     bool(activation), bool(channel_last), lattice)

    def occupancy_queries(self, semantic_logits, density_feature, occ_coords, bda_mat, beta=None):
        """bv2:596-604: (occ_logits [B,K,oz,oy,ox], occ_density [B,1,oz,oy,ox]) on the occ grid
        rotated by bda[:3,:3] (a tiny torch matmul; the two resamplings are HIP kernels)."""
        B = semantic_logits.shape[0]
        if not occ_coords.is_cuda or not (bda_mat is None or bda_mat.is_cuda):
            raise _capi.VampireHipError("occ_coords and bda_mat must be device tensors (no CPU fallback)")
        if occ_coords.dim() != 4 or occ_coords.shape[-1] != 3:
            raise ValueError(f"occ_coords: expected shape [n0, n1, n2, 3], got {tuple(occ_coords.shape)}")
        if bda_mat is not None and (bda_mat.dim() != 3 or bda_mat.shape[0] != B or min(bda_mat.shape[1:]) < 3):
            raise ValueError(f"bda_mat: expected shape ({B}, 4, 4), got {tuple(bda_mat.shape)}")
        # (both volumes and beta before the first of the two resamplings is launched)
        c = self.cfg
        semantic_logits = _chk(_accept_float(semantic_logits, "semantic_logits"),
                               (B, semantic_logits.shape[1], c.vZ, c.vY, c.vX), "semantic_logits")
        density_feature = _chk(_accept_float(density_feature, "density_feature"), (B, 1, c.vZ, c.vY, c.vX),
                               "density_feature")
        if beta is not None:
            _scalar(beta, "beta")
        # R @ c for every grid point as one [P,3] x [3,3] product per sample (the reference's
        # broadcast of 640k 3x3 matmuls, bv2:599, costs 8 ms on the GPU)
        if bda_mat is None:      # the static grid of BaseLSSImpaintor / BaseLSS / BaseBiLinear
            pts = occ_coords.reshape(1, -1, 3).float().expand(B, -1, 3).contiguous()
        else:
            pts = torch.matmul(occ_coords.reshape(1, -1, 3).float(), bda_mat[:, :3, :3].float().transpose(1, 2))
        shp = tuple(occ_coords.shape[:3])
        logits = self.sample_points(semantic_logits, pts, padding="border", lattice=shp)
        dens = self.sample_points(density_feature, pts, activation=True, beta=beta, lattice=shp)
        return logits.reshape(B, -1, *shp), dens.reshape(B, 1, *shp)

    def occupancy_points(self, occ_coords, bda_mat):
        """The occ grid [n0, n1, n2, 3] as the points `point_queries` takes: rotated by bda[:3, :3] per sample (bv2:599)
        -> [B, P, 3], with the torch.matmul of `occupancy_queries` (the same bits); bda_mat None: the static grid of
        BaseLSSImpaintor / BaseLSS / BaseBiLinear -> [1, P, 3], shared by all samples."""
        if not occ_coords.is_cuda or not (bda_mat is None or bda_mat.is_cuda):
            raise _capi.VampireHipError("occ_coords and bda_mat must be device tensors (no CPU fallback)")
        if occ_coords.dim() != 4 or occ_coords.shape[-1] != 3:
            raise ValueError(f"occ_coords: expected shape [n0, n1, n2, 3], got {tuple(occ_coords.shape)}")
        if bda_mat is None:
            return occ_coords.reshape(1, -1, 3).float()
        if bda_mat.dim() != 3 or min(bda_mat.shape[1:]) < 3:
            raise ValueError(f"bda_mat: expected shape (B, 4, 4), got {tuple(bda_mat.shape)}")
        return torch.matmul(occ_coords.reshape(1, -1, 3).float(), bda_mat[:, :3, :3].float().transpose(1, 2))

    def point_queries(self, semantic_logits, density_feature, beta=None, *, points=None, counts=None, sdf=False,
                      occ_points=None, lattice=None):
        """The four point queries of a step (bv2:576-609) in one operator and one autograd node: one forward launch per
        point set, one backward with one cell list that writes each volume's gradient once.  Same bits as the four
        `sample_points` / `occupancy_queries` calls.

        semantic_logits [B, K, Z, Y, X] (K + 1 <= 32), density_feature [B, 1, Z, Y, X] (None when neither `sdf` nor
        `occ_points` asks for it); fp32 or bf16 each, gradients come back in each volume's dtype.
        points: per-sample list of [n_b, 3] ego-frame points, padded here without reading anything back, or a packed
        [B, M, 3] tensor with `counts` (int32 [B] on the device; None: all M rows).  Rows beyond a count are never
        read (they may hold NaN) and their output rows are exact 0; with packed inputs the call can be captured in a
        graph and replayed with other counts.  sdf: also return pts_sdf (bv2:594-595).
        occ_points: [B, P, 3] or [1, P, 3] (`occupancy_points`); lattice: the grid's (n0, n1, n2), a layout hint.
        Returns PointQueries(pts_logits [B, M, K], pts_sdf [B, M], occ_logits [B, K, P], occ_density [B, 1, P]); the
        parts not asked for are None.  occ_density is the sampled density, without the module's tanh."""
        from .queries import point_queries
        return point_queries(self, semantic_logits, density_feature, beta, points=points, counts=counts, sdf=sdf,
                             occ_points=occ_points, lattice=lattice)

    # ------------------------------------------------- producer / consumer glue
    def depth_softmax(self, logits):
        """`mapping_along_depth(src).softmax(dim=1)` (bv2:550): logits [B*N, D, fH, fW] fp32 | bf16
        -> fp32 depth distribution of the same shape (what `lift` takes as `depth`)."""
        return _DepthSoftmaxFn.apply(self, logits)

    def density_gate(self, voxel_output, voxel_density):
        """`voxel_output * bev_density.tanh()` (sdf) / `voxel_output * bev_density` (naive),
        bv2:627-630: [B,C,oZ,oY,oX] x [B,1,oZ,oY,oX] -> [B,C,oZ,oY,oX]."""
        return _DensityGateFn.apply(self, voxel_output, voxel_density)


    def gate_conv1x1_supported(self, C_, oZ, cout):
        return bool(self.vamp.vamp_gate_conv1x1_supported(int(C_), int(oZ), int(cout)))

    def gate_conv1x1(self, voxel_output, voxel_density, weight, bias=None):
        """The density gate and the `voxel_output` 1x1 conv in one kernel (bv2:627-632; SURVEY 8f N2, consumer
        side): voxel_output [B,C,oZ,oY,oX], voxel_density [B,1,oZ,oY,oX], weight [Cout, C*oZ(,1,1)], bias
        [Cout] | None -> [B,Cout,oY,oX] = conv1x1((voxel_output * gate(voxel_density)).reshape(B, C*oZ, oY, oX))."""
        with torch.cuda.device(self.device):
            return _GateConvFn.apply(self, voxel_output, voxel_density, weight, bias)


# ===========================================================================
# autograd glue
# ===========================================================================
class _LiftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp: HotPath, depth, feat, mats, use_depth, grad_mode=True, logits=False):
        c = hp.cfg
        B, N, C_ = feat.shape[:3]
        ctx.logits = logits
        ctx.in_dtypes = (depth.dtype if use_depth else None, feat.dtype)
        feat = _accept_float(feat, "feat")
        if logits:
            # `depth` holds the logits (their own dtype); the kernel writes the fp32 distribution
            lg = _chk(_accept_float(depth, "depth logits"), (B, N, c.D) + tuple(feat.shape[-2:]), "depth logits")
            feat = feat.float()
            depth = torch.empty(lg.shape, dtype=torch.float32, device=lg.device)
        elif use_depth:
            # (checked like every other operand: the kernel reads B * N * D * fH * fW contiguous elements, and the
            # tensor saved for the backward is this one)
            depth = _chk(_accept_float(depth, "depth"), (B, N, c.D) + tuple(feat.shape[-2:]), "depth")
            if depth.dtype != feat.dtype:               # mixed inputs (e.g. fp32 softmax output + half features)
                depth, feat = depth.float(), feat.float()
        code = _dtype_code(feat)
        fhw = tuple(feat.shape[-2:])
        d = hp.lift_desc(B, N, C_, code, use_depth, fhw=fhw)
        # channel-last fp32 features (the memory of a torch.channels_last producer) go in as they are
        # (VAMP_LIFTFWD_FEAT_CHANNEL_LAST: no transposing first launch); anything else is made [B,N,C,fH,fW]-contiguous
        fcl = _is_channel_last(feat) and (not use_depth or logits or depth.dtype == torch.float32)
        ctx.feat_cl = fcl
        if fcl:
            if not feat.is_cuda:
                raise _capi.VampireHipError("feat must be a device tensor (no CPU fallback)")
            if tuple(feat.shape) != (B, N, C_) + fhw:
                raise ValueError(f"feat: expected shape {(B, N, C_) + fhw}, got {tuple(feat.shape)}")
        else:
            feat = _chk(feat, (B, N, C_) + fhw, "feat")
        mats = _mats(mats, B, N, "lift_mats")
        out = torch.empty(B, C_, c.vZ, c.vY, c.vX, dtype=torch.float32, device=feat.device)
        # (the caller's grad mode comes in as an argument: inside forward it is always off and
        # needs_input_grad ignores torch.no_grad(), under which the backward's hit words / prepare
        # pass would be wasted work)
        need_grad = grad_mode and (ctx.needs_input_grad[2] or (use_depth and ctx.needs_input_grad[1]))
        nchunk = (C_ + 15) // 16
        hits = (torch.empty(B, c.vZ, c.vY, c.vX, nchunk, dtype=torch.int64, device=feat.device)
                if need_grad else None)
        ws = hp._lift_workspace(d)
        cur = torch.cuda.current_stream()
        hp._lift_gen += 1
        ctx.cells_key = None
        flags = _capi.VAMP_LIFTFWD_FEAT_CHANNEL_LAST if fcl else 0
        if need_grad and hp.impl["lift_bwd"] == "cell":
            # the forward kernel projects every voxel into every camera anyway: in grad mode it also
            # counts the backward's (voxel, camera) pairs per pixel cell and leaves their taps and depth samples in
            # the workspace, so the backward never projects (a backward whose lists another call has overwritten
            # since -- cells_key below -- builds them itself)
            flags |= _capi.VAMP_LIFTFWD_EMIT_PAIRS
            hp._finish_lift_scan()          # (an earlier forward's deferred scan: its counters must be spent first)
            if hp.impl["defer_lift_scan"]:
                flags |= _capi.VAMP_LIFTFWD_DEFER_SCAN
            if hp._counters.begin("lift", ws.data_ptr(), hp._cnt_range("lift", d)):
                flags |= _capi.VAMP_LIFTFWD_CELLS_CLEAN
            # (the counters are in flight until this call has been issued in full)
            ctx.cells_key = (hp._lift_gen, ws.data_ptr())
        if logits:
            hp.vamp.vamp_lift_forward_logits_ex(d, mats, hp.xs, hp.ys, hp.zs, lg, _dtype_code(lg), feat, depth, out,
                                               hits, ws, ws.numel(), flags, _stream(cur))
        else:
            hp.vamp.vamp_lift_forward_ex(d, mats, hp.xs, hp.ys, hp.zs, depth if use_depth else None, feat, out, hits, ws,
                                        ws.numel(), flags, _stream(cur))
        if flags & _capi.VAMP_LIFTFWD_DEFER_SCAN:
            hp._lift_scan_pending = (d, ws, cur)      # (the counters stay in flight until the scan)
        elif flags & _capi.VAMP_LIFTFWD_EMIT_PAIRS:
            hp._counters.done("lift", ws.data_ptr(), hp._cnt_range("lift", d))      # emit + scan issued: back at zero
        if need_grad:
            ctx.hp, ctx.desc, ctx.use_depth = hp, d, use_depth
            ctx.save_for_backward(depth if use_depth else feat, feat, mats, hits)
        return out

    @staticmethod
    def backward(ctx, g):
        hp, d, use_depth = ctx.hp, ctx.desc, ctx.use_depth
        depth, feat, mats, hits = ctx.saved_tensors
        g = g.contiguous().float()
        if ctx.feat_cl:      # the gradient in the features' own (channel-last) memory layout
            B_, N_, C_, fH_, fW_ = feat.shape
            gfeat = torch.empty(B_, N_, fH_, fW_, C_, dtype=torch.float32, device=feat.device).permute(0, 1, 4, 2, 3)
        else:
            gfeat = torch.empty(feat.shape, dtype=torch.float32, device=feat.device)
        gdepth = (torch.empty(depth.shape, dtype=torch.float32, device=feat.device)
                  if use_depth else None)
        ws = hp._lift_workspace(d)
        hp._finish_lift_scan()              # (nobody has run the forward's deferred scan: a lift without a render forward)
        fresh = ctx.cells_key == (hp._lift_gen, ws.data_ptr())       # the forward's pair cells are still in the workspace
        hp._lift_gen += 1                                              # the backward consumes the prepared counters
        if hp.impl["lift_bwd"] == "v1":
            flags = _capi.VAMP_LIFTBWD_SPLAT                           # (takes neither the cells nor the logits)
        else:
            flags = ((_capi.VAMP_LIFTBWD_CELLS_VALID if fresh else 0)
                     | (_capi.VAMP_LIFTBWD_LOGITS if ctx.logits else 0))
        if ctx.feat_cl:
            flags |= _capi.VAMP_LIFTBWD_FEAT_CHANNEL_LAST
        flags |= {1: _capi.VAMP_LIFTBWD_WPP1, 4: _capi.VAMP_LIFTBWD_WPP4,
                  16: _capi.VAMP_LIFTBWD_WPP16}.get(hp.impl["lift_wpp"], 0)
        hp._counters.begin("lift", ws.data_ptr(), hp._cnt_range("lift", d))
        hp.vamp.vamp_lift_backward_ex(d, mats, hp.xs, hp.ys, hp.zs, depth if use_depth else None, feat, g, hits,
                                     gdepth, gfeat, ws, ws.numel(), flags, _stream())
        if hp.impl["lift_bwd"] == "cell":
            hp._counters.done("lift", ws.data_ptr(), hp._cnt_range("lift", d))     # the gather has re-zeroed the fill's cursors
        if ctx.logits and hp.impl["lift_bwd"] == "v1":
            # (the cross-check implementation returns the gradient of the distribution)
            gdepth = depth * (gdepth - (depth * gdepth).sum(2, keepdim=True))
        gd = gdepth.to(ctx.in_dtypes[0]) if use_depth else None
        return None, gd, gfeat.to(ctx.in_dtypes[1]), None, None, None, None


class _LiftDenseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp: HotPath, ff, mats):
        c = hp.cfg
        B, N, C_, D = ff.shape[:4]
        use_depth = D > 1
        d = hp.lift_desc(B, N, C_, _capi.VAMP_F32, use_depth, fhw=tuple(ff.shape[-2:]))
        d.D = D
        ff = _chk(ff.float(), (B, N, C_, D) + tuple(ff.shape[-2:]), "frustum_feats")
        mats = _mats(mats, B, N, "lift_mats")
        out = torch.empty(B, C_, c.vZ, c.vY, c.vX, dtype=torch.float32, device=ff.device)
        nchunk = (C_ + 15) // 16
        hits = (torch.empty(B, c.vZ, c.vY, c.vX, nchunk, dtype=torch.int64, device=ff.device)
                if ctx.needs_input_grad[1] else None)
        hp.vamp.vamp_lift_forward_dense(d, mats, hp.xs, hp.ys, hp.zs, ff, out, hits, _stream())
        if ctx.needs_input_grad[1]:
            ctx.hp, ctx.desc, ctx.shape = hp, d, ff.shape
            ctx.save_for_backward(mats, hits)
        return out

    @staticmethod
    def backward(ctx, g):
        hp, d = ctx.hp, ctx.desc
        mats, hits = ctx.saved_tensors
        g = g.contiguous().float()
        gff = torch.zeros(ctx.shape, dtype=torch.float32, device=g.device)
        hp.vamp.vamp_lift_backward_dense(d, mats, hp.xs, hp.ys, hp.zs, g, hits, gff, _stream())
        return None, gff, None


def render_forward_plan(train, two, prep_ok, direct, ert, merged=False):
    """The C calls of one render forward in issue order: [(op, stream, flags, waits, records)].

    op: "term" (termination table), "pack" (channel-last copy of the volumes), "cam" (camera branch: the one
    kernel when `direct`, else the planned march), "prep" (the backward's geometry-only prepare pass), "bev",
    "render" (camera tiles + BEV column blocks in ONE launch, vamp_render_forward_merged: stands for "cam" + "bev";
    only with `merged`, which the caller gives when direct and ert hold and the library supports the shapes).
    stream: "cur" | "side"; flags: beyond the op's base flags; waits / records: names of events.
    `two`: a side stream is available; `prep_ok`: the cell-list backward will follow on matrices (no explicit
    geometry, not the v1 splat); `direct` / `ert`: one-kernel camera forward / early ray termination.
    Every schedule holds exactly one "bev" and one "cam"; the rest is what the measured timelines of
    DESIGN.md 7g-7h settled on (one table instead of four hand-unrolled branches)."""
    F = _capi
    if not (direct and ert):
        merged = False
    if merged and not train:
        return [("render", "cur", 0, (), ())]
    if merged and train and prep_ok:
        # training: the camera tiles also draw the backward's cell ranks, and the call finishes the prepare step (the cell
        # scan, together with the lift's deferred one) behind the launch -- one launch + one small one on ONE stream where
        # rounds 3 - 5 ran the camera kernel, the BEV forward and the prepare pass as three launches on two
        # (the scan on the side stream, with the backward's camera chain behind it there and its BEV chain here, so that
        # the BEV chain would start beside it: 0.411 against 0.395 ms -- it stays on this stream)
        return [("render", "cur", F.VAMP_RENDERFWD_RANK, (), ()),
                ("prep", "cur", F.VAMP_CAMPREP_RANKED, (), ())]
    if train and two and prep_ok and direct:
        # the camera kernel (which leaves the termination table), then the BEV forward; beside them, once the
        # table is there, the prepare pass
        return [("cam", "cur", F.VAMP_CAMFWD_DIRECT, (), ("table",)),
                ("prep", "side", F.VAMP_CAMPREP_TERM_VALID, ("table",), ()),
                ("bev", "cur", 0, (), ())]
    if train and two and prep_ok and ert:
        # planned march: the side stream takes what only the camera branch needs later -- table, copy, prepare
        # pass -- this stream the BEV forward and, once table and copy are there, the march
        return [("term", "side", 0, (), ()),
                ("pack", "side", F.VAMP_CAMFWD_TERM_VALID | F.VAMP_CAMFWD_PACK_ONLY, (), ("packed",)),
                ("prep", "side", F.VAMP_CAMPREP_TERM_VALID, (), ()),
                ("bev", "cur", 0, (), ()),
                ("cam", "cur", F.VAMP_CAMFWD_TERM_VALID | F.VAMP_CAMFWD_PACKED_VALID, ("packed",), ())]
    if direct and not train:
        # forward only (BEV issued first: second, it starts behind the camera kernel and finds the CUs taken)
        return [("bev", "side" if two else "cur", 0, (), ()), ("cam", "cur", F.VAMP_CAMFWD_DIRECT, (), ())]
    steps, camf = [], (F.VAMP_CAMFWD_DIRECT if direct else 0)
    if ert and not direct:
        steps.append(("term", "cur", 0, (), ("table",)))
        camf |= F.VAMP_CAMFWD_TERM_VALID
    prep = train and two and prep_ok and not direct
    # without early termination the march is the long kernel of the step, and a BEV forward beside it costs it more
    # than it hides (207 us beside, 150 alone).  The BEV forward therefore OPENS the side stream: it runs beside the
    # channel-last copy in front of the march (a kernel of 1.5 TB/s: latency, not bytes), with the prepare pass behind
    # it -- replayed step 0.788 against 0.808 ms with the BEV forward behind the march (rounds 4 - 6)
    bev_first = prep and not ert
    if bev_first or not prep:
        steps.append(("bev", "side" if two else "cur", 0, (), ()))
    if prep:
        steps.append(("prep", "side", F.VAMP_CAMPREP_TERM_VALID if ert else 0, ("table",) if ert else (), ()))
    if prep and not bev_first:
        steps.append(("bev", "side", 0, (), ()))
    steps.append(("cam", "cur", camf, (), ()))
    return steps


def render_backward_plan(two, matrices, cell_impl, fresh, cells, samples, ert, packed, bev_cell, bev_saved, tab_valid):
    """The C calls of one render backward in issue order: [(op, stream, flags, waits, records)].

    op: "cam" (vamp_render_camera_backward_acc) | "bev" (vamp_render_bev_backward_ex); stream: "cur" | "side";
    flags: the call's COMPLETE flag word; waits / records: names of events.  Only a "cam" op waits, and its wait is not a
    stream wait: the event goes into the call as its wait_event argument and the library places the wait itself (in
    front of the gather).
    `two`: a side stream is available; `matrices`: no explicit geometry; `cell_impl` / `bev_cell`: the cell-list camera /
    BEV backward (not the v1 splats).  `fresh`: the render workspace is untouched since this forward -- what the
    forward left there (`cells`: cell lists, `samples`: sample rows, `ert`: it ran with early termination and left the
    table, `packed`: channel-last copy) is promised to the library only then.  `bev_saved` / `tab_valid`: the BEV
    workspace still holds this forward's samples / a split pair's axis tables (cell-list BEV backward only).
    The camera and the BEV branch add into the same three gradient buffers: the first writer overwrites (a BEV call
    with OVERWRITE_CAM, or a camera call without ACCUMULATE), the second accumulates.  Three schedules: two streams
    with both backwards split in parts, one stream BEV first, and -- v1 splat or explicit geometry, whose camera
    backward only overwrites -- camera first."""
    F = _capi
    valid = 0 if ert else F.VAMP_CAMBWD_NO_ERT          # (how the forward marched, whatever has become of its leavings)
    if fresh:
        valid |= ((F.VAMP_CAMBWD_PACKED_VALID if packed else 0) | (F.VAMP_CAMBWD_CELLS_VALID if cells else 0)
                  | (F.VAMP_CAMBWD_SAMPLES_VALID if samples and cell_impl else 0)
                  | (F.VAMP_CAMBWD_TERM_VALID if ert else 0))
    bev = F.VAMP_BEVBWD_OVERWRITE_BASE | (F.VAMP_BEVBWD_SAVED_VALID if bev_saved and bev_cell else 0)
    if not (matrices and cell_impl):
        return [("cam", "cur", valid | (0 if cell_impl else F.VAMP_CAMBWD_SPLAT), (), ()),
                ("bev", "cur", bev, (), ())]
    cam, bev = valid | F.VAMP_CAMBWD_ACCUMULATE, bev | F.VAMP_BEVBWD_OVERWRITE_CAM
    if not two:
        # (TABLE_VALID is sent beside a part flag only: `tab_valid` speaks of the two tables of a split pair)
        return [("bev", "cur", bev, (), ()), ("cam", "cur", cam, (), ())]
    # Two streams: the BEV branch writes the buffers on the side stream while the camera branch marches its rays and
    # sorts its samples on this one (ray pass and the heavy cells' per-corner sums: neither touches the gradient
    # buffers); the camera gather then waits for the BEV event and adds on top.  The pass-through (grad_base) gather of
    # the BEV branch is issued behind the event: nobody waits for grad_base, so it runs beside the camera gather
    # instead of in front of it.
    # Issue order: the camera chain FIRST.  It is the longer chain and the lift backward follows it, and a replayed
    # graph keeps the branch whose first node was created first on the queue of the nodes around the fork -- the other
    # branch pays the cross-queue hand-over (5 - 13 us at its start, and again where it joins).
    # (cfg-B replayed: 0.3625 - 0.370 ms/step against 0.3735 with the BEV chain issued first.)
    if tab_valid and bev_cell:
        bev |= F.VAMP_BEVBWD_TABLE_VALID
    return [("cam", "cur", cam | F.VAMP_CAMBWD_PART_RAY | F.VAMP_CAMBWD_PART_HEAVY, (), ()),
            ("bev", "side", bev | F.VAMP_BEVBWD_SKIP_BASE, (), ("bev",)),
            ("bev", "side", bev | F.VAMP_BEVBWD_ONLY_BASE, (), ()),
            ("cam", "cur", cam | F.VAMP_CAMBWD_PART_GATHER, ("bev",), ())]


class _RenderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp: HotPath, dens, sem, base, rgb, beta, geom, mats, grad_mode=True):
        c = hp.cfg
        # will a backward follow?  (grad_mode is the caller's: inside forward it is always off, and
        # needs_input_grad ignores torch.no_grad())
        train = grad_mode and any(ctx.needs_input_grad)
        B = dens.shape[0]
        N = (geom if geom is not None else mats).shape[1]
        C_ = base.shape[1]
        ctx.in_dtypes = tuple(t.dtype for t in (dens, sem, base, rgb))
        dens, sem, base, rgb = (_accept_float(t, nm) for t, nm in zip(
            (dens, sem, base, rgb), ("density_feature", "semantic_logits", "voxel_features", "rgb")))
        if len({t.dtype for t in (dens, sem, base, rgb)}) > 1:
            dens, sem, base, rgb = (t.float() for t in (dens, sem, base, rgb))
        d = hp.render_desc(B, N, _dtype_code(dens), C_)
        vshape = (c.vZ, c.vY, c.vX)
        dens = _chk(dens, (B, 1) + vshape, "density_feature")
        sem = _chk(sem, (B, c.num_classes) + vshape, "semantic_logits")
        base = _chk(base, (B, C_) + vshape, "voxel_features")
        rgb = _chk(rgb, (B, 3) + vshape, "rgb")
        if geom is not None:
            geom = _chk(geom.float(), (B, N, c.D, c.fH, c.fW, 3), "geom_xyz")
        else:
            mats = _chk(mats.float(), (B, N, 3, 4, 4), "render_mats")
        ctx.beta_shape = beta.shape
        beta = _scalar(beta, "beta")
        dev, f32 = dens.device, torch.float32
        K = c.num_classes
        CO = C_ + (K if c.cat_seg else 0)
        if CO == 0:
            # (the library takes C = 0 beside cat_seg only: voxel_output would have no channels, and its forward needs one)
            raise ValueError("mid_channels = 0 needs cat_seg: voxel_output would have no channels")
        rgb_p = torch.empty(B, N, 3, c.fH, c.fW, dtype=f32, device=dev)
        seg_p = torch.empty(B, N, K, c.fH, c.fW, dtype=f32, device=dev)
        dep_p = torch.empty(B, N, 1, c.fH, c.fW, dtype=f32, device=dev)
        bev_rgb = torch.empty(B, 3, c.oY, c.oX, dtype=f32, device=dev)
        bev_seg = torch.empty(B, K, c.oY, c.oX, dtype=f32, device=dev)
        bev_h = torch.empty(B, 1, c.oY, c.oX, dtype=f32, device=dev)
        vdens = torch.empty(B, 1, c.oZ, c.oY, c.oX, dtype=f32, device=dev)
        vout = torch.empty(B, CO, c.oZ, c.oY, c.oX, dtype=f32, device=dev)
        # training: the camera forward also keeps every inside sample's gathered values (tile-major rows, 256
        # contiguous bytes per tile, depth index and channel), and the backward's per-ray pass reads them back
        # instead of repeating the 8-tap gathers
        save = bool(train and geom is None and hp.impl["save_rows"] and hp.impl["cam_bwd"] != "v1" and (c.D - 1) <= 128)
        ws = hp._render_workspace(d, rows=save)
        # which camera forward: the one kernel with early termination, or copy + planned march (with the
        # termination pre-pass or without) -- from the switches, or ("auto") from what the rays did lately
        ert, direct = hp._camera_forward_choice(geom is None and (c.D - 1) <= 128, geom is None)
        # the two branches share only their inputs: in a training step they (and the prepare pass) use two
        # streams; forward-only calls stay on one unless the caller captures them into a graph (fwd_overlap)
        cur = torch.cuda.current_stream()
        side = hp._side_stream() if (train or hp.impl["fwd_overlap"]) else None
        prep_ok = geom is None and hp.impl["cam_bwd"] != "v1"
        # camera tiles + BEV column blocks in one launch where the library takes the shapes (it checks the heights
        # hp.ozs_host against the BEV kernel's plane slabs itself)
        merged = bool(direct and ert and hp.impl["fwd_merged"] and hp.impl["bev_fused"] and
                      hp.vamp.vamp_render_forward_merged_supported(d, hp.ozs_host))
        # training calls take the one launch (camera tiles + rank pass + BEV blocks) while the camera tiles are at most
        # four rounds of the chip's workgroup slots: cfg-B, replayed step, merged against the three launches on two
        # streams -- 1 / 2 / 3 samples per GPU 0.395 / 0.710 / 1.03 against 0.410 / 0.723 / 1.05 ms, 4 samples equal,
        # 8 samples 2.69 against 2.63 (a full chip hides the prepare pass beside the BEV forward better than it
        # fills the camera tiles' tail)
        if merged and train and B * N * ((c.fH + 7) // 8) * ((c.fW + 7) // 8) > int(hp.impl.get("merged_tiles", 4096)):
            merged = False
        plan = render_forward_plan(train, side is not None, prep_ok, direct, ert, merged)
        bev_flags = 0 if hp.impl["bev_fused"] else _capi.VAMP_BEVFWD_TWO_KERNELS
        bev_save = train and hp.impl["bev_bwd"] != "v1"
        ws_bev = hp._workspace("bev", hp.vamp.vamp_render_bev_workspace_bytes(d)) if bev_save else None
        cam_base = 0 if ert else _capi.VAMP_CAMFWD_NO_ERT
        streams, events = {"cur": cur, "side": side}, {}
        ctx.cells, ctx.ert, ctx.bev_key = False, ert, None
        # the backward's d loss / d beta accumulator is zeroed by the FORWARD: as the first node of the backward the
        # one-element fill sat alone on the step's critical path (5 us + the same again of hand-over behind a kernel
        # that short).  The merged launch zeroes the word itself; the other schedules with a fill on their side stream
        gbeta_in_launch = train and any(op == "render" for op, *_ in plan)
        ctx.gbeta0 = torch.empty(1, dtype=f32, device=dev) if gbeta_in_launch else None
        # (a fork / join with nothing on the other side still costs a replayed graph a barrier: only plans that use the
        # side stream touch it)
        if side is not None and not any(where == "side" for _, where, *_ in plan):
            side = None
            streams["side"] = None
        if side is not None:
            side.wait_stream(cur)
        if train and not gbeta_in_launch:
            if side is not None:
                with torch.cuda.stream(side):
                    ctx.gbeta0 = torch.zeros(1, dtype=f32, device=dev)
                ctx.gbeta0.record_stream(cur)
            else:
                ctx.gbeta0 = torch.zeros(1, dtype=f32, device=dev)
        for op, where, flags, waits, records in plan:
            st = streams[where]
            for w in waits:
                st.wait_event(events[w])
            if op == "term":
                hp.vamp.vamp_render_camera_terminate(d, mats, hp.us, hp.vs, hp.ds, beta, dens, ws, ws.numel(),
                                                    _stream(st))
            elif op in ("cam", "pack"):
                keep = _capi.VAMP_CAMFWD_SAVE_SAMPLES if (save and op == "cam") else 0
                hp.vamp.vamp_render_camera_forward_ex(d, geom, mats, hp.us, hp.vs, hp.ds, hp.camera_mids, beta, dens,
                                                     sem, rgb, rgb_p, seg_p, dep_p, ws, ws.numel(),
                                                     cam_base | flags | keep, _stream(st))
            elif op == "prep":
                ranked = bool(flags & _capi.VAMP_CAMPREP_RANKED)       # (the forward drew the ranks: scan + work lists only)
                pend = hp._lift_scan_pending
                pflags = flags | (0 if ranked else hp._cam_clean_flag(d, ws))
                if pend is not None and pend[2] == cur:
                    # a lift forward's pair cells are due too: both scans in one launch.  (The lift ran on `cur`; this
                    # op's stream is `cur` or the side stream, which has waited for `cur` above and which `cur` waits
                    # for below: the lift backward is ordered behind the scan either way.)
                    hp._lift_scan_pending = None
                    hp.vamp.vamp_render_camera_prepare_with_lift(
                        d, mats, hp.us, hp.vs, hp.ds, ws, ws.numel(), pflags, pend[0], pend[1], pend[1].numel(),
                        _stream(st))
                    hp._counters.done("lift", pend[1].data_ptr(), hp._cnt_range("lift", pend[0]))
                else:
                    hp.vamp.vamp_render_camera_prepare_ex(d, mats, hp.us, hp.vs, hp.ds, ws, ws.numel(), pflags,
                                                         _stream(st))
                hp._counters.done("render", ws.data_ptr(), hp._cnt_range("render", d))
                ctx.cells = True
            elif op == "render":
                hp.vamp.vamp_render_forward_merged(
                    d, mats, hp.us, hp.vs, hp.ds, hp.camera_mids, hp.oxs, hp.oys, hp.ozs, hp.ozs_host, hp.bev_mids, beta,
                    dens, sem, rgb, base, rgb_p, seg_p, dep_p, bev_rgb, bev_seg, bev_h, vdens, vout, ws, ws.numel(),
                    ws_bev, ws_bev.numel() if bev_save else 0, ctx.gbeta0 if train else None,
                    (_capi.VAMP_RENDERFWD_SAVE_SAMPLES if save else 0) | (_capi.VAMP_RENDERFWD_BEV_SAVE if bev_save else 0)
                    | flags | (_capi.VAMP_RENDERFWD_COUNTERS_CLEAN if (flags & _capi.VAMP_RENDERFWD_RANK) and hp._cam_clean_flag(d, ws) else 0),
                    _stream(st))
                # (with VAMP_RENDERFWD_RANK the counters stay "in flight" until the "prep" op behind has scanned them)
            else:
                hp.vamp.vamp_render_bev_forward_ex(d, hp.oxs, hp.oys, hp.ozs, hp.bev_mids, beta, dens, sem, rgb, base,
                                                  bev_rgb, bev_seg, bev_h, vdens, vout, hp.ozs_host, ws_bev,
                                                  ws_bev.numel() if bev_save else 0,
                                                  (_capi.VAMP_BEVFWD_SAVE if bev_save else 0) | bev_flags, _stream(st))
            if op in ("render", "bev"):
                hp._bev_gen += 1
                ctx.bev_key = (hp._bev_gen, ws_bev.data_ptr()) if bev_save else None
            for r in records:
                events[r] = torch.cuda.Event()
                events[r].record(st)
        if side is not None:
            cur.wait_stream(side)
        hp._camera_forward_probe(d, ws, (mats, beta, dens), ert, geom is None, cur)
        ctx.samples = save
        ctx.hp, ctx.desc = hp, d
        # the workspace now holds the termination table, the channel-last copy of (dens, sem, rgb) unless the
        # one kernel ran, and the cell lists if a prepare pass did; the backward reuses them if no other render
        # call has touched the workspace in between
        hp._pack_gen += 1
        ctx.pack_key = None if (direct and not train) else (hp._pack_gen, ws.data_ptr())
        ctx.packed = not direct                 # (the one-kernel forward makes no channel-last copy)
        ctx.has_geom = geom is not None
        ctx.save_for_backward(dens, sem, base, rgb, beta, geom if geom is not None else mats)
        return rgb_p, seg_p, dep_p, bev_rgb, bev_seg, bev_h, vdens, vout

    @staticmethod
    def backward(ctx, g_rgb, g_seg, g_dep, g_brgb, g_bseg, g_bh, g_vd, g_vo):
        hp, d = ctx.hp, ctx.desc
        dens, sem, base, rgb, beta, gm = ctx.saved_tensors
        geom, mats = (gm, None) if ctx.has_geom else (None, gm)
        f32 = torch.float32
        cont = lambda t: None if t is None else t.contiguous().float()
        g_rgb, g_seg, g_dep, g_brgb, g_bseg, g_bh, g_vd, g_vo = map(
            cont, (g_rgb, g_seg, g_dep, g_brgb, g_bseg, g_bh, g_vd, g_vo))
        ws = hp._render_workspace(d, rows=ctx.samples)
        ws_bev = hp._workspace("bev", hp.vamp.vamp_render_bev_workspace_bytes(d))
        # every gradient buffer is written in full by the calls below (the BEV branch overwrites,
        # the camera branch adds, or the other way round): no zero fills
        gb = torch.empty(base.shape, dtype=f32, device=dens.device)
        gd = torch.empty(dens.shape, dtype=f32, device=dens.device)
        gs = torch.empty(sem.shape, dtype=f32, device=dens.device)
        gr = torch.empty(rgb.shape, dtype=f32, device=dens.device)
        gbeta, ctx.gbeta0 = getattr(ctx, "gbeta0", None), None        # (a second backward of the same graph zeroes its own)
        if gbeta is None:
            gbeta = torch.zeros(1, dtype=f32, device=dens.device)

        # the axis tables in the BEV workspace depend on the grids only (constants of this object):
        # valid once both halves of a split pair have written theirs into this very buffer
        tab_key = (ws_bev.data_ptr(), d.B)
        cur, side = torch.cuda.current_stream(), hp._side_stream()
        cell_impl, bev_cell = hp.impl["cam_bwd"] != "v1", hp.impl["bev_bwd"] != "v1"
        fresh = ctx.pack_key == (hp._pack_gen, ws.data_ptr())
        plan = render_backward_plan(
            two=side is not None, matrices=geom is None, cell_impl=cell_impl,
            fresh=fresh, cells=ctx.cells, samples=ctx.samples, ert=ctx.ert,
            packed=ctx.packed, bev_cell=bev_cell, bev_saved=ctx.bev_key == (hp._bev_gen, ws_bev.data_ptr()),
            tab_valid=hp._bev_tab_key == tab_key)
        cnt_rng = hp._cnt_range("render", d)
        relists = cell_impl and geom is None and ctx.cells and not fresh
        if not cell_impl or geom is not None or not ctx.cells:
            # the v1 splat keeps a packed gradient copy where the cell lists live, and a backward that builds
            # its own cell lists may stop half way: either way the counters there are no longer known zero
            hp._counters.spoil("render")
        elif relists:
            # the forward's cell lists are gone: this backward counts and scans again (zero-filling first), and the
            # counters are in flight until its calls have been issued in full
            hp._counters.begin("render", ws.data_ptr(), cnt_rng)
        hp._pack_gen += 1                                       # the backward scribbles after the copy only,
        ctx.pack_key = None                                     # but a second backward must not assume so
        streams, events = {"cur": cur, "side": side}, {}
        forked = any(where == "side" for _, where, *_ in plan)
        if forked:
            side.wait_stream(cur)
        for op, where, flags, waits, records in plan:
            st = streams[where]
            if op == "cam":
                # (the event is the call's own argument: the library waits for it in front of its gather)
                wait = C.c_void_p(events[waits[0]].cuda_event) if waits else None
                hp.vamp.vamp_render_camera_backward_acc(d, geom, mats, hp.us, hp.vs, hp.ds, hp.camera_mids, beta, dens,
                                                       sem, rgb, g_rgb, g_seg, g_dep, gd, gs, gr, gbeta, ws, ws.numel(),
                                                       flags, wait, _stream(st))
            else:
                hp.vamp.vamp_render_bev_backward_ex(d, hp.oxs, hp.oys, hp.ozs, hp.bev_mids, beta, dens, sem, rgb, base,
                                                   g_brgb, g_bseg, g_bh, g_vd, g_vo, gd, gs, gr, gb, gbeta,
                                                   hp.ozs_host if bev_cell else None, ws_bev, ws_bev.numel(), flags,
                                                   _stream(st))
                if flags & _capi.VAMP_BEVBWD_ONLY_BASE:
                    hp._bev_tab_key = tab_key                   # (both halves of the split pair have been issued)
            for r in records:
                events[r] = torch.cuda.Event()
                events[r].record(st)
        if forked:
            cur.wait_stream(side)
        if relists:
            hp._counters.done("render", ws.data_ptr(), cnt_rng)
        grad_beta = gbeta.reshape(ctx.beta_shape) if hp.cfg.density_mode == "sdf" else None
        dt = ctx.in_dtypes
        return (None, gd.to(dt[0]), gs.to(dt[1]), gb.to(dt[2]), gr.to(dt[3]), grad_beta, None, None, None)


class _SamplePointsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp: HotPath, volume, points, beta, padding, mask_outside, activation, channel_last,
                lattice=None):
        c = hp.cfg
        B, C_ = volume.shape[:2]
        ctx.in_dtype = volume.dtype
        volume = _chk(_accept_float(volume, "volume"), (B, C_, c.vZ, c.vY, c.vX), "volume")
        P = points.shape[1]
        points = _chk(points.float(), (B, P, 3), "points")
        d = _capi.VampSampleDesc()
        d.B, d.C, d.Z, d.Y, d.X = B, C_, c.vZ, c.vY, c.vX
        for i, bnd in enumerate((c.x_bound_seg, c.y_bound_seg, c.z_bound_seg)):
            d.lo[i] = bnd[0]
            d.span[i] = bnd[1] - bnd[0]
        if padding not in ("zeros", "border"):
            raise ValueError("padding must be 'zeros' or 'border'")
        d.padding = _capi.VAMP_PAD_BORDER if padding == "border" else _capi.VAMP_PAD_ZEROS
        d.mask_outside = 1 if mask_outside else 0
        d.activation = 1 if activation else 0
        d.density_mode = _density_code(c)
        d.sdf_bias, d.beta_min = c.sdf_bias, 1e-4
        d.channel_last_out = 1 if channel_last else 0
        d.in_dtype = _dtype_code(volume)
        for i in range(3):
            d.lattice[i] = int(lattice[i]) if lattice is not None else 0
        ctx.beta_shape = beta.shape
        beta = _scalar(beta, "beta")
        out = torch.empty((B, P, C_) if channel_last else (B, C_, P), dtype=torch.float32,
                          device=volume.device)
        hp.vamp.vamp_sample_points_forward(d, volume, beta, points, P, out, _stream())
        ctx.hp, ctx.desc, ctx.P, ctx.activation = hp, d, P, activation
        ctx.save_for_backward(volume, points, beta)
        return out

    @staticmethod
    def backward(ctx, g):
        hp, d, P = ctx.hp, ctx.desc, ctx.P
        volume, points, beta = ctx.saved_tensors
        g = g.contiguous().float()
        gvol = torch.empty(volume.shape, dtype=torch.float32, device=volume.device)
        gbeta = torch.zeros(1, dtype=torch.float32, device=volume.device)
        ws = hp._workspace("sample", hp.vamp.vamp_sample_points_workspace_bytes(d, P))
        hp.vamp.vamp_sample_points_backward(d, volume, beta, points, P, g, gvol, gbeta, ws, ws.numel(), _stream())
        grad_beta = (gbeta.reshape(ctx.beta_shape)
                     if (ctx.activation and hp.cfg.density_mode == "sdf") else None)
        return None, gvol.to(ctx.in_dtype), None, grad_beta, None, None, None, None, None


class _DepthSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp: HotPath, logits):
        if logits.dim() < 3:
            raise ValueError("logits: expected [images, D, ...]")
        if not logits.is_cuda:
            raise _capi.VampireHipError("logits must be a device tensor (no CPU fallback)")
        ctx.in_dtype = logits.dtype
        logits = _accept_float(logits, "logits").contiguous()
        images, D = logits.shape[:2]
        HW = logits[0, 0].numel()
        out = torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
        if logits.numel():
            hp.vamp.vamp_depth_softmax_forward(images, D, HW, logits, _dtype_code(logits), out, _stream())
        ctx.hp, ctx.dims = hp, (images, D, HW)
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        g = g.contiguous().float()
        gx = torch.empty_like(p)
        if p.numel():
            ctx.hp.vamp.vamp_depth_softmax_backward(*ctx.dims, p, g, gx, _stream())
        return None, gx.to(ctx.in_dtype)


class _DensityGateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp: HotPath, vo, vd):
        if not (vo.is_cuda and vd.is_cuda):
            raise _capi.VampireHipError("voxel_output / voxel_density must be device tensors (no CPU fallback)")
        B, C_ = vo.shape[:2]
        vd = _chk(_accept_float(vd, "voxel_density").float(), (B, 1) + tuple(vo.shape[2:]), "voxel_density")
        vo = _accept_float(vo, "voxel_output").float().contiguous()
        cells = vd[0].numel()
        mode = _density_code(hp.cfg)
        out = torch.empty_like(vo)
        if vo.numel():
            hp.vamp.vamp_density_gate_forward(B, C_, cells, mode, vo, vd, out, _stream())
        ctx.hp, ctx.dims = hp, (B, C_, cells, mode)
        ctx.save_for_backward(vo, vd)
        return out

    @staticmethod
    def backward(ctx, g):
        vo, vd = ctx.saved_tensors
        g = g.contiguous().float()
        gvo, gvd = torch.empty_like(vo), torch.empty_like(vd)
        if vo.numel():
            ctx.hp.vamp.vamp_density_gate_backward(*ctx.dims, g, vo, vd, gvo, gvd, _stream())
        return None, gvo, gvd


class _GateConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp: HotPath, vo, vd, weight, bias):
        need_device("gate_conv1x1", vo, vd, weight)
        B, C_, oZ = vo.shape[:3]
        plane = tuple(vo.shape[3:])
        cells = int(math.prod(plane))
        cout = weight.shape[0]
        vd = _chk(_accept_float(vd, "voxel_density").float(), (B, 1, oZ) + plane, "voxel_density")
        vo = _accept_float(vo, "voxel_output").float().contiguous()
        w = _chk(_accept_float(weight, "weight").float().reshape(cout, -1), (cout, C_ * oZ), "weight")
        bs = None if bias is None else _chk(bias.float(), (cout,), "bias")
        mode = _density_code(hp.cfg)
        out = torch.empty((B, cout) + plane, dtype=torch.float32, device=vo.device)
        dims = (B, C_, oZ, cells, cout, mode)
        hp.vamp.vamp_gate_conv1x1_forward(*dims, vo, vd, w, bs, out, _stream())
        ctx.hp, ctx.dims, ctx.wshape, ctx.has_bias = hp, dims, tuple(weight.shape), bias is not None
        ctx.dtypes = (weight.dtype, None if bias is None else bias.dtype)
        ctx.save_for_backward(vo, vd, w)
        return out

    @staticmethod
    def backward(ctx, g):
        hp = ctx.hp
        vo, vd, w = ctx.saved_tensors
        g = g.contiguous().float()
        gvo, gvd, gw = torch.empty_like(vo), torch.empty_like(vd), torch.empty_like(w)
        gb = torch.empty(w.shape[0], dtype=torch.float32, device=w.device) if ctx.has_bias else None
        B, C_, oZ, cells, cout, mode = ctx.dims
        ws = hp._workspace("gate_conv", hp.vamp.vamp_gate_conv1x1_workspace_bytes(C_, oZ, cout))
        hp.vamp.vamp_gate_conv1x1_backward(*ctx.dims, g, vo, vd, w, gvo, gvd, gw, gb, ws, ws.numel(), _stream())
        return (None, gvo, gvd, gw.reshape(ctx.wshape).to(ctx.dtypes[0]),
                None if gb is None else gb.to(ctx.dtypes[1]))
