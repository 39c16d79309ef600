"""The BEV branch of the renderer across the det-grid geometry that picks its code paths -- heights oZ, the det step
against the voxel spacing, lattices shifted against or leaving the volume, ragged and narrow det grids, the seg grid's
Z (the pass-through gather's z segments), K, the density mode and bf16 volumes -- against the oracle evaluated in
float64 (oracle/aten_oracle.py, compute_dtype): every output and every gradient, on each forced path.

One axis moves at a time from CFG_TINY (B = 2, six cameras); where the det lattice grows in z the seg grid's z bound
grows with it, except in the cases that are about leaving the volume.  Scene, upstream gradients and bars are those of
tests/test_render_shape_sweep.py.  The CPU tests at the end map the cases through mirrors of the BEV launchers' dispatch,
fail if a forward body, a backward gather body, the zero path or an LDS regime is reached by no case, and compare the
library's own host-side answers (merged launch supported, BEV workspace bytes, the backward's plan field by field) with
the mirrors -- the plan also on descriptors above 2 GB, which no GPU test can allocate."""
import ctypes as C
import dataclasses
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import aten_oracle as O
from vampire_amd import _capi, synthetic
from vampire_amd.config import CFG_TINY, axis_cells
from vampire_amd.geometry import PathGeometry, axis_centres, render_matrices
from test_hip_parity import NAMES, hot, _upstream
from test_render_shape_sweep import (BETA_BAR, GRAD_BAR, OUT_BAR, VOLS, _Calls, bf16_excess, rel_err)

F64 = torch.float64
f32 = np.float32

# ---------------------------------------------------------------------------------------------------- the constants
K_MAX_T = 3               # kMaxT: lattice points within one voxel's support per axis (render_bev.hip)
BEV_MAX_OZ = 64           # kBevMaxOZ / kFusedMaxOZ
FUSED_MAX_NP = 40         # kFusedMaxNP (render_bev_fused_dev.hpp)
QS_MAX_WAVES = 16         # kQsMaxWaves: the saved q-scan's waves (one per height up to 16)
COL_G = 4                 # VAMP_COLG
PLAN_MAX = 128            # kPlanMax
LDS_RAISE = 60 * 1024     # the non-saved q kernel raises its dynamic-LDS limit above this
I32 = 0x7fffffff


def bound(lo, n, step):
    """(lo, hi, step) with axis_cells == n (hi nudged up past int()'s truncation where lo + n * step rounds low)."""
    hi = lo + n * step
    while axis_cells((lo, hi, step)) < n:
        hi = math.nextafter(hi, math.inf)
    assert axis_cells((lo, hi, step)) == n, (lo, hi, step, n)
    return (lo, hi, step)


TINY = CFG_TINY
EX = (TINY.x_bound_seg[1] - TINY.x_bound_seg[0]) / (TINY.vX - 1)      # voxel spacing in x: 12.8 / 15
EZ = (TINY.z_bound_seg[1] - TINY.z_bound_seg[0]) / (TINY.vZ - 1)      # and in z: 1.0


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    x_det: tuple = TINY.x_bound_det
    y_det: tuple = TINY.y_bound_det
    z_det: tuple = TINY.z_bound_det
    x_seg: tuple = TINY.x_bound_seg
    y_seg: tuple = TINY.y_bound_seg
    z_seg: tuple = TINY.z_bound_seg
    K: int = 5
    C: int = 4
    cat_seg: bool = False
    mode: str = "sdf"
    bf16: bool = False
    want: tuple = ()          # predicates of plan() the case exists for (checked on the CPU)

    @property
    def cfg(self):
        return dataclasses.replace(TINY, x_bound_det=self.x_det, y_bound_det=self.y_det, z_bound_det=self.z_det,
                                   x_bound_seg=self.x_seg, y_bound_seg=self.y_seg, z_bound_seg=self.z_seg,
                                   num_classes=self.K, mid_channels=self.C, cat_seg=self.cat_seg,
                                   density_mode=self.mode)


def heights(oZ, step=0.8, Z=None):
    """oZ heights from z = 0 up, the seg grid's z bound grown with them (Z planes of 0.8 m from z = -2)."""
    Z = Z or max(5, oZ + 3)
    return dict(z_det=bound(-0.4 * step / 0.8, oZ, step), z_seg=bound(-2.0, Z, 0.8))


def x_ratio(r):
    step = r * EX
    return dict(x_det=bound(-6.4, int(12.8 / step), step))


def z_ratio(r):
    step = r * EZ
    return dict(z_det=bound(-2.0, max(1, int(4.0 / step)), step))


HEIGHTS = [1, 2, 16, 17, 40, 60, 61, 64]
RATIOS = [2, 1.5, 1, 0.7, 0.6]
SEG_Z = [5, 8, 9, 16, 17]
NARROW = Case("narrow-4x200", x_det=bound(-1.6, 4, 0.8), y_det=bound(-80.0, 200, 0.8), y_seg=bound(-80.0, 200, 0.8),
              want=("fits", "scan-partials-exceed-saved"))
ABOVE = dict(z_det=bound(2.8, 3, 0.8))
CASES = ([Case(f"oZ{n}", **heights(n), want=("fits",)) for n in HEIGHTS]
         + [Case("oZ64-fused", **heights(64, step=0.4, Z=35), want=("fused", "generic"))]
         + [Case(f"x{r}", **x_ratio(r), want=("generic",) if r < 2 / 3 else ("fits",)) for r in RATIOS]
         + [Case(f"z{r}", **z_ratio(r), want=("generic",) if r < 2 / 3 else ("fits",)) for r in RATIOS]
         + [Case("shift-half", x_det=bound(-6.4 + EX / 2, 15, 0.8), y_det=bound(-6.4 + EX / 2, 15, 0.8),
                 z_det=bound(-0.9, 3, 0.8), want=("fits",)),
            Case("partial-xy", x_det=bound(-10.4, 16, 0.8), y_det=bound(-2.4, 16, 0.8), want=("fits",)),
            Case("partial-above-z", z_det=bound(0.4, 4, 0.8), want=("fits",)),
            Case("above-z-sdf", **ABOVE, want=("zero",)),
            Case("above-z-naive", **ABOVE, mode="naive", want=("zero",)),
            Case("outside-x", x_det=bound(7.2, 16, 0.8), want=("fits",))]
         + [Case(f"oX{n}", x_det=bound(-0.4 * n, n, 0.8), want=("fits",)) for n in (1, 3)]
         + [Case(f"oX{n}", x_det=bound(-6.4, n, 0.8), x_seg=bound(-6.4, n, 0.8), want=("fits",)) for n in (65, 100)]
         + [Case("oY24", y_det=bound(-6.4, 24, 0.8), y_seg=bound(-6.4, 24, 0.8)),
            Case("oY7", y_det=bound(-2.8, 7, 0.8)),
            NARROW]
         + [Case(f"segZ{Z}-catseg", z_det=bound(-2.0, Z, 0.8), z_seg=bound(-2.0, Z, 0.8), cat_seg=True,
                 want=("fits",)) for Z in SEG_Z]
         + [Case(f"segZ{Z}-C0-catseg", z_det=bound(-2.0, Z, 0.8), z_seg=bound(-2.0, Z, 0.8), C=0, cat_seg=True,
                 want=("fits", "zsegments")) for Z in (9, 16)]
         + [Case("K18", K=18, want=("qscan21",)), Case("K18-oZ64", K=18, **heights(64), want=("qscan21",)),
            Case("naive", mode="naive"), Case("naive-x0.6", mode="naive", **x_ratio(0.6)),
            Case("naive-oZ64", mode="naive", **heights(64))]
         + [Case("bf16", bf16=True), Case("bf16-x0.6", bf16=True, **x_ratio(0.6)),
            Case("bf16-oZ61", bf16=True, **heights(61)), Case("bf16-K18", K=18, bf16=True),
            Case("bf16-segZ16-catseg", bf16=True, z_det=bound(-2.0, 16, 0.8), z_seg=bound(-2.0, 16, 0.8),
                 cat_seg=True)])
CASE_BY_NAME = {c.name: c for c in CASES}

# the forced paths: HotPath.impl switches ("between": a second training forward between the forward and its backward,
# so that the backward finds the BEV workspace holding a later forward's samples)
CELL = dict(cam_direct=True, ert=True, fwd_merged=True, bev_fused=True, cam_bwd="cell", bev_bwd="cell", overlap=True)
PATHS = {
    "merged": dict(CELL),
    "two-launch": dict(CELL, fwd_merged=False),
    "bev-two-kernel": dict(CELL, bev_fused=False),
    "unsaved": dict(CELL, between=True),
    "accumulate": dict(CELL, overlap=False, cam_bwd="v1"),
    "bev-v1": dict(CELL, bev_bwd="v1"),
}


# ---------------------------------------------------------------------------------------------------- mirrors of the dispatch
def desc(case, B=2):
    from vampire_amd.ops import render_desc
    return render_desc(case.cfg, B, TINY.num_cams, _capi.VAMP_BF16 if case.bf16 else _capi.VAMP_F32)


def ozs_host(case):
    return [f32(v) for v in axis_centres(case.z_det).tolist()]


def planes_alloc(d):
    """render_common.hpp: bev_planes_alloc (fp32, as the C++ evaluates it)."""
    per = abs(f32(d.det_step[2])) * f32(d.Z - 1) / f32(d.span[2])
    return int(math.ceil(f32(d.oZ - 1) * per)) + 4


def tap0(d, pos):
    """The floor z tap of a height (bev_fused_heights_fit / the backward's z range)."""
    g = ((f32(pos) - f32(d.lo[2])) / f32(d.span[2])) * f32(2.0) - f32(1.0)
    f = ((g + f32(1.0)) / f32(2.0)) * f32(d.Z - 1)
    return f, int(math.floor(f))


def heights_fit(d, ozs):
    """render_common.hpp: bev_fused_heights_fit."""
    if d.oZ < 1:
        return False
    taps = []
    for pos in ozs:
        if not abs(pos) <= 3.0e38:
            return False
        f, i0 = tap0(d, pos)
        if not abs(f) < 1.0e9:
            return False
        taps.append(i0)
    return max(taps) + 1 - min(taps) + 2 <= planes_alloc(d)


def fused_supported(d):
    """render_bev_fused.hip: bev_fwd_fused_supported."""
    V = d.Z * d.Y * d.X
    es = 4 if d.in_dtype == _capi.VAMP_F32 else 2
    cmax = max(d.K, d.C)
    CO = d.C + (d.K if d.cat_seg else 0)
    omax = max(CO, d.K + 3) * d.oZ * d.oY * d.oX * 4
    return (d.oZ <= BEV_MAX_OZ and d.X >= 2 and max(cmax, 3) * V * es < I32 and omax < I32
            and planes_alloc(d) <= FUSED_MAX_NP)


def merged_supported(d, ozs):
    """render_fwd_merged.hip: render_fwd_merged_supported, and vamp_render_forward_merged_supported's height check."""
    return (d.D - 1 <= PLAN_MAX and fused_supported(d) and d.oZ > 0 and d.oY > 0 and d.oX > 0
            and heights_fit(d, ozs))


def scan_blocks(d, saved):
    """render_common.hpp: bev_scan_blocks -- the d beta partials of bev_qscan_saved_kernel / bev_scan_kernel."""
    if saved:
        return (d.oY * d.oX + 63) // 64 * d.B
    return (d.oX + 63) // 64 * ((d.oY + 3) // 4) * d.B


def align_up(n, a=256):
    return (n + a - 1) // a * a


def ws_needed(d):
    """render_common.hpp: bev_workspace -- the BEV workspace both scans need: Q, Wb, DS0 | two axis tables | the larger count of beta partials | density
    samples and composited channels' samples the forward keeps."""
    one = align_up(d.B * d.oZ * d.oY * d.oX * 4)
    tab = align_up(2 * (d.X + d.Y + d.Z) * 16)
    return 3 * one + 2 * tab + align_up(max(scan_blocks(d, True), scan_blocks(d, False)) * 4) + (d.K + 4) * one


def bwd_plan(d, ozs):
    """render_bev.hip: bev_backward_plan's numbers for the cell backward (flags aside: lib_plan)."""
    taps = [tap0(d, pos)[1] for pos in ozs]
    z_lo, z_hi = max(0, min(taps)), min(d.Z - 1, max(taps) + 1)
    p = dict(z_lo=z_lo, z_hi=z_hi, zero=z_lo > z_hi, q_lds=d.oZ * 4 * 64 * 4, qs_lds=4 * d.oZ * 64 * 4,
             qscan=21 if d.K + 3 == 21 and d.B * 21 * d.oZ * d.oY * d.oX * 4 < I32 else 0)
    fits = True
    for a, n in enumerate((d.X, d.Y, d.Z)):
        e = f32(d.span[a]) / f32(n - 1)
        if not f32(d.det_step[a]) > 0 or int(math.floor(f32(2.0) * e / f32(d.det_step[a]))) + 1 > K_MAX_T:
            fits = False
    if d.oZ > BEV_MAX_OZ or any(not ozs[k] > ozs[k - 1] for k in range(1, d.oZ)):
        fits = False
    p["fits"] = fits
    p["comp_ok"] = d.B * d.K * d.Z * d.Y * d.X * 4 < I32 and d.B * d.oZ * d.oY * d.oX * 4 < I32
    p["pass_ok"] = (d.B * (d.C + (d.K if d.cat_seg else 0)) * d.oZ * d.oY * d.oX * 4 < I32
                    and d.B * d.C * d.Z * d.Y * d.X * 4 < I32)
    wgs = (d.Y * d.X + 255) // 256 * d.B * ((d.C + COL_G - 1) // COL_G)
    nseg = min(max(1, (1250 + wgs - 1) // max(1, wgs)), max(1, d.Z // 4))
    zseg = (d.Z + nseg - 1) // nseg
    p["nseg"], p["zseg"] = (d.Z + zseg - 1) // zseg, zseg
    return p


PLAN_FIELDS = [n for n, _ in _capi.VampBevBackwardPlan._fields_]
ERR_HEIGHTS = "at most 64 det-grid heights"
ERR_HALVES = "ONLY_BASE and SKIP_BASE exclude each other"
ERR_OFFSETS = "tensor too large for the 32-bit offsets of the BEV gather"


def lib_plan(d, ozs, flags):
    """render_bev.hip: bev_backward_plan -- what vamp_render_bev_backward_plan is to answer for (d, ozs, flags): every
    field of VampBevBackwardPlan (grids and reserved words as lists), or the message of the refusal.  ozs None: the
    caller gave no host heights."""
    A = _capi
    only, skip = bool(flags & A.VAMP_BEVBWD_ONLY_BASE), bool(flags & A.VAMP_BEVBWD_SKIP_BASE)
    ow_base, ow_cam = bool(flags & A.VAMP_BEVBWD_OVERWRITE_BASE), bool(flags & A.VAMP_BEVBWD_OVERWRITE_CAM)
    saved, sdf = bool(flags & A.VAMP_BEVBWD_SAVED_VALID), d.density_mode == A.VAMP_DENSITY_SDF_LAPLACE
    p = {n: [0] * 3 if n.endswith("_grid") else [0] * 6 if n == "reserved" else 0 for n in PLAN_FIELDS}
    if ozs is None:
        # the float-atomic splat behind its zero fills; of a split pair the SKIP_BASE call does it all
        p.update(path=A.VAMP_BEVPLAN_PATH_NOOP if only else A.VAMP_BEVPLAN_PATH_V1,
                 zero_cam=int(ow_cam and not only), zero_base=int(ow_base and not only))
        return p
    p["path"] = A.VAMP_BEVPLAN_PATH_CELL
    if d.oZ > BEV_MAX_OZ:
        return ERR_HEIGHTS
    if only and skip:
        return ERR_HALVES
    b = bwd_plan(d, ozs)
    p.update(z_lo=b["z_lo"], z_hi=b["z_hi"], outside=int(b["zero"]), beta_parts=scan_blocks(d, saved))
    # the scan: not in the ONLY_BASE half; outside the volume only for the sdf density's d beta
    if not only and (sdf or not b["zero"]):
        gx = (d.oX + 63) // 64
        if saved:
            p.update(scan=A.VAMP_BEVPLAN_SCAN_QSCAN21 if b["qscan"] == 21 else A.VAMP_BEVPLAN_SCAN_QSCAN0,
                     scan_grid=[(d.oY * d.oX + 63) // 64, d.B, 1], scan_waves=min(d.oZ, QS_MAX_WAVES),
                     scan_lds=b["qs_lds"])
        else:
            p.update(scan=A.VAMP_BEVPLAN_SCAN_Q_SCAN, q_grid=[gx, d.oY, d.B], scan_grid=[gx, (d.oY + 3) // 4, d.B],
                     scan_waves=4, scan_lds=b["q_lds"], raise_lds=int(b["q_lds"] > LDS_RAISE))
    if b["zero"]:
        # each half of a pair zeroes what it owns; the d beta partials are added up right behind the scan
        early = A.VAMP_BEVPLAN_BETA_EARLY if p["scan"] else A.VAMP_BEVPLAN_BETA_NONE
        p.update(zero_cam=int(ow_cam and not only), zero_base=int(ow_base and not skip), beta_reduce=early,
                 beta_reduce_no_vo=early)
        return p
    p["fits"] = int(b["fits"])
    beta_due = sdf and not skip                 # (the SKIP_BASE half leaves the partials to the ONLY_BASE half)
    if not b["fits"]:
        # the generic gather adds to all four tensors at once: the ONLY_BASE half has nothing to launch but the reduction
        launch = A.VAMP_BEVPLAN_BETA_LAUNCH if beta_due else A.VAMP_BEVPLAN_BETA_NONE
        p.update(generic=int(not only), zero_cam=int(ow_cam and not only), zero_base=int(ow_base and not only),
                 beta_reduce=launch, beta_reduce_no_vo=launch)
        return p
    if d.B * max(d.K, d.C) * d.Z * d.Y * d.X >= I32 or d.B * (d.C + d.K) * d.oZ * d.oY * d.oX >= I32:
        return ERR_OFFSETS
    p.update(build_table=int(not flags & A.VAMP_BEVBWD_TABLE_VALID), table=int(only), nseg=b["nseg"], zseg=b["zseg"],
             comp_ok=int(b["comp_ok"]), pass_ok=int(b["pass_ok"]))
    launches = []                               # the column-gather launches that can carry the beta tail, in order
    if not only:
        p.update(comp_body=A.VAMP_BEVPLAN_BODY_COMP if b["comp_ok"] else A.VAMP_BEVPLAN_BODY_COL,
                 comp_overwrite=int(ow_cam), seg_gather=int(bool(d.cat_seg)))
        launches.append((A.VAMP_BEVPLAN_BETA_TAIL_COMP, False))
    if not skip and d.C > 0:
        p.update(base_body=A.VAMP_BEVPLAN_BODY_PASS if b["pass_ok"] else A.VAMP_BEVPLAN_BODY_COL,
                 base_overwrite=int(ow_base),
                 base_body_no_vo=A.VAMP_BEVPLAN_BODY_ZERO if ow_base else A.VAMP_BEVPLAN_BODY_NONE)
        launches.append((A.VAMP_BEVPLAN_BETA_TAIL_BASE, True))       # (runs only with g_voxel_output)
    if beta_due:
        p["beta_reduce"] = launches[0][0] if launches else A.VAMP_BEVPLAN_BETA_LAUNCH
        no_vo = [where for where, needs_vo in launches if not needs_vo]
        p["beta_reduce_no_vo"] = no_vo[0] if no_vo else A.VAMP_BEVPLAN_BETA_LAUNCH
    return p


def big_descriptors():
    """Descriptors no GPU test can allocate (pure numbers here): [(name, d, ozs, flags)].  The seg grid grows to
    20 x 2000 x 2000 inside CFG_TINY's bounds (finer voxels: the lattice still fits the column gathers), or the det
    grid to 2000 x 2000 columns."""
    def make(K=5, C=4, B=2, seg=None, det=None, oZ=None):
        d = desc(Case("big", K=K, C=C), B=B)
        if seg:
            d.Z, d.Y, d.X = seg
        if det:
            d.oY, d.oX = det
        ozs = ozs_host(Case("big"))
        if oZ:
            d.oZ, ozs = oZ, [f32(-1.9 + 0.05 * k) for k in range(oZ)]
        return d, ozs
    SEG = (20, 2000, 2000)
    both = _capi.VAMP_BEVBWD_OVERWRITE_BASE | _capi.VAMP_BEVBWD_OVERWRITE_CAM
    return [("comp-col", *make(K=5, C=1, seg=SEG), both),                    # B K Z Y X 4 = 3.2e9, B C Z Y X 4 = 6.4e8
            ("pass-col", *make(K=1, C=4, seg=SEG), both),                    # B K Z Y X 4 = 6.4e8, B C Z Y X 4 = 2.6e9
            ("qscan0-21ch", *make(K=18, B=4, det=(2000, 2000)), both | _capi.VAMP_BEVBWD_SAVED_VALID),
            ("offsets", *make(K=18, B=4, seg=SEG), both),                    # B K Z Y X = 5.8e9 elements
            ("both-halves", *make(), both | _capi.VAMP_BEVBWD_ONLY_BASE | _capi.VAMP_BEVBWD_SKIP_BASE),
            ("oZ65", *make(oZ=65), both)]


def plan(case, path="merged"):
    """What the library runs for one case on one path: forward body, backward bodies, and the predicates the cases
    are chosen for."""
    d, ozs = desc(case), ozs_host(case)
    p = PATHS[path]
    b = bwd_plan(d, ozs)
    fused = fused_supported(d) and heights_fit(d, ozs)
    mrg = merged_supported(d, ozs)
    if p["fwd_merged"] and p["bev_fused"] and mrg:
        fwd = "merged"
    else:
        fwd = "fused" if (p["bev_fused"] and fused) else "two-kernel"
    bodies = set()
    saved = not p.get("between") and p["bev_bwd"] != "v1"
    if p["bev_bwd"] == "v1":
        bodies.add("v1")
    elif b["zero"]:
        bodies.add("zero")
        if d.density_mode == _capi.VAMP_DENSITY_SDF_LAPLACE:       # (the d beta term still needs the scan)
            bodies.add(f"qscan{b['qscan']}" if saved else "q")
    else:
        bodies.add(f"qscan{b['qscan']}" if saved else "q")
        if b["fits"]:
            bodies.add("comp-overwrite" if p["cam_bwd"] != "v1" else "comp-accumulate")
            if case.cat_seg:
                bodies.add("col-seg" if b["nseg"] == 1 else "col-seg-zsegments")
            if d.C > 0:
                bodies.add("pass")
        else:
            bodies.add("generic")
    lds = None
    if "q" in bodies:
        lds = ("q", b["q_lds"] > LDS_RAISE)
    elif any(x.startswith("qscan") for x in bodies):
        lds = ("qscan", b["qs_lds"] > LDS_RAISE)
    preds = {"fused": fused, "merged": mrg, "fits": b["fits"] and not b["zero"], "generic": not b["fits"] and not b["zero"],
             "zero": b["zero"], "zsegments": b["nseg"] > 1, f"qscan{b['qscan']}": True,
             "scan-partials-exceed-saved": align_up(scan_blocks(d, True) * 4) < scan_blocks(d, False) * 4}
    return dict(fwd=fwd, bodies=bodies, lds=lds, preds=preds, **b)


# ---------------------------------------------------------------------------------------------------- scenes, oracle
@functools.lru_cache(maxsize=None)
def scene(case, vseed=17):
    """CPU tensors: (cfg, render_mats [B,N,3,4,4], volumes (fp32, bf16-rounded for bf16 cases), beta); the low-x half of
    the density volume in the "empty" regime (tests/test_render_shape_sweep.py)."""
    cfg = case.cfg
    s2e, intrin, ida = synthetic.camera_rig(cfg, 2, jitter=1.0, seed=5)
    rm = render_matrices(s2e, intrin, ida, synthetic.bda_matrix(2, rot_deg=5.0))
    vols = list(synthetic.render_inputs(cfg, 2, seed=vseed))
    d = vols[0].clone()
    d[..., : d.shape[-1] // 2] *= 0.4
    vols[0] = d
    if case.bf16:
        vols = [v.bfloat16().float() for v in vols]
    return cfg, rm, vols, 0.1


@functools.lru_cache(maxsize=None)
def oracle_render(case, vseed=17, seed=4545):
    """float64 oracle: the eight outputs, the four volume gradients, grad_beta (None in naive mode) and the sum of the
    magnitudes of grad_beta's terms (one per sample and BEV cell), for the upstream of _upstream(seed)."""
    cfg, rm, vols, beta_v = scene(case, vseed)
    terms, sdf = [], O.density_sdf

    def per_term_beta(s, beta_param, bias, beta_min=1e-4):
        b = beta_param.expand(s.shape)
        b.retain_grad()
        terms.append(b)
        return sdf(s, b, bias, beta_min)
    geo = PathGeometry(cfg)
    geom = torch.nan_to_num(O.frustum_to_ego(geo.frustum, None, None, None, None, prepared=rm), -1e3)
    v64 = [v.double().requires_grad_(True) for v in vols]
    beta = torch.tensor(beta_v, dtype=F64, requires_grad=True) if cfg.density_mode == "sdf" else None
    O.density_sdf = per_term_beta
    try:
        outs = O.render(geom, *v64, seg_bounds=(cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg),
                        output_coords=geo.output_coords, camera_mids=geo.camera_mids, bev_mids=geo.bev_mids,
                        d_far=cfg.d_bound[1], z_step_det=cfg.z_bound_det[2], num_classes=cfg.num_classes,
                        density_mode=cfg.density_mode, beta_param=beta, sdf_bias=cfg.sdf_bias, cat_seg=cfg.cat_seg,
                        compute_dtype=F64)
    finally:
        O.density_sdf = sdf
    ups = [u.cpu().double() for u in _upstream([o.shape for o in outs], seed, "cpu")]
    torch.autograd.backward(outs, ups)
    if beta is None:
        assert not terms
        return [o.detach() for o in outs], [v.grad for v in v64], None, None
    assert len(terms) == 2                          # camera branch, BEV branch
    scale = sum(float(t.grad.abs().sum()) for t in terms)
    assert abs(sum(float(t.grad.sum()) for t in terms) - float(beta.grad)) <= 1e-9 * scale
    return [o.detach() for o in outs], [v.grad for v in v64], float(beta.grad), scale


def large_grid(cfg):
    return max(cfg.vX, cfg.vY, cfg.vZ) > 32


@functools.lru_cache(maxsize=None)
def bars(case):
    """(output bar, gradient bar).  Where a seg axis has n > 32 voxels the fp32 tap coordinate f = (g + 1) / 2 * (n - 1)
    of the reference's formulation -- the kernels form it the same way -- carries up to 2^-24 (n - 1) of rounding
    (1.2e-5 at n = 200), and the reference's own fp32 evaluation (fp32_reference) is off the float64 one by as much as
    the kernels are: outputs 4.2e-5 / 1.9e-5 / 1.5e-5 / 1.0e-5 / 6.7e-6 at oX = 4, oY = 200 / oX = 100 / oZ = 60 /
    oZ = 64 / oZ = 40, gradients 2.8e-5 / 1.1e-5 / 1.0e-5 / 1.0e-5 on the first four.  On such a case a bar grows by
    four of those roundings, 4 * 2^-24 (n - 1), where the fp32 reference's error uses up more than half of it."""
    cfg = case.cfg
    if not large_grid(cfg):
        return OUT_BAR, GRAD_BAR
    t = 4 * 2.0 ** -24 * (max(cfg.vX, cfg.vY, cfg.vZ) - 1)
    ro, rg, _, _ = oracle_render(case)
    o32, g32 = fp32_reference(case)
    e_out = max(out_excess(cfg, nm, o, ro) for nm, o in zip(NAMES, o32))
    e_grad = max(rel_err(g, r) for g, r in zip(g32, rg))
    return OUT_BAR + (t if e_out > OUT_BAR / 2 else 0.0), GRAD_BAR + (t if e_grad > GRAD_BAR / 2 else 0.0)


def fp32_allowance(cfg, nm, ref_outs):
    """Per-element absolute allowance of one output for the fp32 rounding of the density activation and the alphas,
    in sdf mode.  f(s; beta) = (0.5 + 0.5 sign(t) expm1(-|t| / beta)) / beta cancels to 2^-24 / beta_eff of absolute
    error where the sample is empty: f(0; 0.1) = 2.3e-4, and a det lattice in empty space holds nothing larger, so
    max |ref| is that small.  alpha = 1 - exp(-sigma dz) cancels to 2^-24 where sigma dz is small, so bev_height =
    sum_j alpha_j T_j mid_j takes 2^-24 (1 + dz / beta_eff) sum_j T_j |mid_j| (T_j: the float64 transmittance in front
    of height j).  The fp32 reference's own errors against these allowances, with the lattice above the volume / beside
    it in x: voxel_density 9.9e-8 / 9.9e-8 (6.0e-7), bev_height 7.0e-7 / 9.3e-8 (6.4e-6 / 8.6e-7).  A 1 % change of
    either fails there (test_fp32_allowance_covers_the_reference_not_a_change)."""
    if cfg.density_mode != "sdf" or nm not in ("voxel_density", "bev_height_preds"):
        return 0.0
    u, beta_eff = 2.0 ** -24, 0.1 + 1e-4
    if nm == "voxel_density":
        return u / beta_eff
    dz = cfg.z_bound_det[2]
    sd = ref_outs[NAMES.index("voxel_density")].double() * dz                # [B, 1, oZ, oY, oX], top-down
    T = torch.exp(-(torch.cumsum(sd, dim=2) - sd))
    mids = torch.flip(axis_centres(cfg.z_bound_det), dims=[0]).double().abs()   # bev_mids, top-down
    return u * (1 + dz / beta_eff) * (T * mids[None, None, :, None, None]).sum(dim=2)


def out_excess(cfg, nm, out, ref_outs):
    """max (|out - ref| - fp32_allowance)+ / max |ref| of one output (the allowance is 0 but for voxel_density and
    bev_height in sdf mode)."""
    ref = ref_outs[NAMES.index(nm)]
    a, b = out.detach().cpu().double(), ref.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    return float(((a - b).abs() - fp32_allowance(cfg, nm, ref_outs)).clamp_min(0).max()) / max(float(b.abs().max()), 1e-30)


def out_err(case, nm, out, ref_outs):
    """(error, bar) of one output (depth_preds: plus three fp32 roundings of sum w ~ 1 times d_far)."""
    cfg = case.cfg
    bar = bars(case)[0]
    if nm == "depth_preds":
        bar += 3 * 1.2e-7 * cfg.d_bound[1] / max(float(ref_outs[NAMES.index(nm)].abs().max()), 1e-30)
    return out_excess(cfg, nm, out, ref_outs), bar


class _Run:
    """One training forward on a HotPath, its backward later."""

    def __init__(self, hp, case, dev, vseed=17, seed=4545):
        self.case, self.vseed, self.seed, self.dev = case, vseed, seed, dev
        cfg, rm, vols, beta_v = scene(case, vseed)
        dt = torch.bfloat16 if case.bf16 else torch.float32
        self.lv = [v.to(dev, dt).requires_grad_(True) for v in vols]
        self.beta = torch.tensor(beta_v, device=dev, requires_grad=True) if cfg.density_mode == "sdf" else None
        self.outs = hp.render(*self.lv, self.beta, render_mats=rm.to(dev))

    def backward(self):
        torch.autograd.backward(self.outs, _upstream([o.shape for o in self.outs], self.seed, self.dev))

    def errors(self, prefix=""):
        cfg = self.case.cfg
        ref_outs, ref_grads, ref_gbeta, gbeta_scale = oracle_render(self.case, self.vseed, self.seed)
        errs = {}
        for nm, o, r in zip(NAMES, self.outs, ref_outs):
            errs[f"{prefix}train {nm}"] = out_err(self.case, nm, o, ref_outs)
        for k, v, r in zip(VOLS, self.lv, ref_grads):
            assert v.grad.dtype == self.lv[0].dtype
            errs[f"{prefix}grad_{k}"] = ((bf16_excess if self.case.bf16 else rel_err)(v.grad, r), bars(self.case)[1])
        if ref_gbeta is not None:
            errs[f"{prefix}grad_beta"] = (abs(float(self.beta.grad) - ref_gbeta) / gbeta_scale, BETA_BAR)
        return errs


def run_path(case, path, dev):
    """One forced path on one case: (errors {what: (err, bar)}, calls).  A no-grad forward, then a training forward
    and its backward on one HotPath (with a second training forward in between on the "unsaved" path)."""
    cfg, rm, vols, beta_v = scene(case)
    hp = hot(cfg, dev)
    hp.impl.update({k: v for k, v in PATHS[path].items() if k != "between"})
    calls = hp.lib = _Calls(hp.lib)
    dt = torch.bfloat16 if case.bf16 else torch.float32
    ref_outs = oracle_render(case)[0]
    with torch.no_grad():
        nog = hp.render(*[v.to(dev, dt) for v in vols], torch.tensor(beta_v, device=dev) if cfg.density_mode == "sdf"
                        else None, render_mats=rm.to(dev))
    errs = {f"no-grad {nm}": out_err(case, nm, o, ref_outs) for nm, o in zip(NAMES, nog)}
    run = _Run(hp, case, dev)
    if PATHS[path].get("between"):
        _Run(hp, case, dev)
    run.backward()
    errs.update(run.errors())
    return errs, calls


def check_calls(case, path, calls):
    """The BEV calls that ran are those of the path (and, where the geometry is outside a launch's limits, of the
    documented fallback: the merged launch falls back to the two launches, i.e. a BEV forward call of its own)."""
    p, pl = PATHS[path], plan(case, path)
    names = [n for n, _ in calls.log]
    mrg = calls.flags("vamp_render_forward_merged", -2)
    bev_f = calls.flags("vamp_render_bev_forward_ex", -2)
    bwd = [a for n, a in calls.log if n == "vamp_render_bev_backward_ex"]
    n_fwd = 3 if p.get("between") else 2
    if pl["fwd"] == "merged" and p["cam_bwd"] != "v1":
        assert len(mrg) == n_fwd and not bev_f, names
    elif pl["fwd"] == "merged":
        # the v1 splat takes no cell lists (render_forward_plan): the no-grad forward is the merged launch, the
        # training forward the one-kernel camera forward and a BEV forward call of its own (the one-kernel BEV forward)
        cam = calls.flags("vamp_render_camera_forward_ex", -2)
        assert len(mrg) == 1 and len(bev_f) == n_fwd - 1, names
        assert len(cam) == n_fwd - 1 and all(f & _capi.VAMP_CAMFWD_DIRECT for f in cam), (names, cam)
        assert not any(f & _capi.VAMP_BEVFWD_TWO_KERNELS for f in bev_f), bev_f
    else:
        assert not mrg and len(bev_f) == n_fwd, names
        assert all(bool(f & _capi.VAMP_BEVFWD_TWO_KERNELS) == (not p["bev_fused"]) for f in bev_f), bev_f
    assert bwd, "no BEV backward ran"
    for a in bwd:
        flags = a[-2]
        assert (a[-5] is None) == (p["bev_bwd"] == "v1"), names
        if p["bev_bwd"] != "v1":
            assert bool(flags & _capi.VAMP_BEVBWD_SAVED_VALID) == (not p.get("between")), flags
            assert bool(flags & _capi.VAMP_BEVBWD_OVERWRITE_CAM) == (p["cam_bwd"] != "v1"), flags


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bev_grid_sweep_against_float64_oracle(dev, case):
    """Each forced path: the eight outputs (no-grad and training forward), the four volume gradients and grad_beta
    against the float64 oracle; the BEV calls made are those of the path or of its documented fallback."""
    bad = []
    for path in PATHS:
        errs, calls = run_path(case, path, dev)
        check_calls(case, path, calls)
        bad += [f"{path} {what}: {e:.3e} > {b:.1e}" for what, (e, b) in errs.items() if not e <= b]
    assert not bad, f"{case.name}:\n" + "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [NARROW, Case("tiny")], ids=lambda c: c.name)
def test_interleaved_forwards_and_backwards(dev, case):
    """Forward A, forward B, backward A, backward B on one HotPath: A's backward finds B's samples in the BEV workspace
    and runs the non-saved scan, whose d beta partials must not land on B's samples; B's backward then reads them."""
    hp = hot(case.cfg, dev)
    calls = hp.lib = _Calls(hp.lib)
    a = _Run(hp, case, dev, vseed=17, seed=4545)
    b = _Run(hp, case, dev, vseed=29, seed=4646)
    a.backward()
    b.backward()
    flags = calls.flags("vamp_render_bev_backward_ex", -2)
    assert len(flags) == 4, flags                   # each backward: the SKIP_BASE and ONLY_BASE calls
    assert [bool(f & _capi.VAMP_BEVBWD_SAVED_VALID) for f in flags] == [False, False, True, True], flags
    errs = {**a.errors("A "), **b.errors("B ")}
    bad = [f"{what}: {e:.3e} > {bar:.1e}" for what, (e, bar) in errs.items() if not e <= bar]
    assert not bad, f"{case.name}:\n" + "\n".join(bad)


# ---------------------------------------------------------------------------------------------------- CPU
def test_heights_above_the_limit_are_refused():
    """oZ = 65 is refused where the HotPath is made: a ValueError naming the limit, before the library is loaded or a
    device touched (the device given here is never used)."""
    from vampire_amd.ops import HotPath
    cfg = Case("oZ65", **heights(65)).cfg
    assert cfg.oZ == 65
    with pytest.raises(ValueError, match="at most 64 det-grid heights"):
        HotPath(cfg, "cuda:0")


def test_cases_hit_their_predicates():
    """Each case's geometry is what it is named for: its heights, its det step against the voxel spacing, the
    predicates it exists for; and the lattice stays inside the volume in z except where leaving it is the point."""
    for c in CASES:
        pl = plan(c)
        for w in c.want:
            assert pl["preds"].get(w), (c.name, w, pl)
        cfg = c.cfg
        assert cfg.oZ <= BEV_MAX_OZ and cfg.oX >= 1 and cfg.oY >= 1, c.name
        zs = axis_centres(cfg.z_bound_det)
        inside = bool(((zs >= cfg.z_bound_seg[0]) & (zs <= cfg.z_bound_seg[1])).all())
        assert inside == (c.name not in ("partial-above-z", "above-z-sdf", "above-z-naive")), c.name
    for n in HEIGHTS:
        assert CASE_BY_NAME[f"oZ{n}"].cfg.oZ == n
    for r in RATIOS:
        for ax, e, i in (("x", EX, 0), ("z", EZ, 2)):
            det = CASE_BY_NAME[f"{ax}{r}"].cfg
            assert abs(det.to_dict()[f"{ax}_bound_det"][2] / e - r) < 1e-6
    assert [CASE_BY_NAME[f"segZ{Z}-catseg"].cfg.vZ for Z in SEG_Z] == SEG_Z
    assert [plan(CASE_BY_NAME[f"segZ{Z}-catseg"])["nseg"] for Z in SEG_Z] == [1, 2, 2, 4, 4]
    assert NARROW.cfg.oX == 4 and NARROW.cfg.oY == 200
    assert {CASE_BY_NAME[f"oX{n}"].cfg.oX for n in (1, 3, 65, 100)} == {1, 3, 65, 100}
    assert CASE_BY_NAME["oY24"].cfg.oY == 24 and CASE_BY_NAME["oY7"].cfg.oY == 7
    # large heights: the one-kernel BEV forward supported at one, not at another
    big = [plan(c)["preds"]["fused"] for c in CASES if c.cfg.oZ >= 40]
    assert True in big and False in big
    assert {c.mode for c in CASES} == {"sdf", "naive"}
    # the wider bar of large seg grids stays off the cases of the ratio, offset, z-segment and channel axes
    large = {c.name for c in CASES if large_grid(c.cfg)}
    assert large == {"oZ40", "oZ60", "oZ61", "oZ64", "oZ64-fused", "oX65", "oX100", "narrow-4x200", "K18-oZ64",
                     "naive-oZ64", "bf16-oZ61"}, sorted(large)
    # ... and of those, only where the reference's own fp32 rounding needs it
    assert {c.name for c in CASES if bars(c)[0] > OUT_BAR} == {"oZ40", "oZ60", "oZ64", "oX100", "narrow-4x200",
                                                               "K18-oZ64"}
    assert {c.name for c in CASES if bars(c)[1] > GRAD_BAR} == {"oZ60", "oZ64", "oX100", "narrow-4x200"}


@functools.lru_cache(maxsize=None)
def fp32_reference(case):
    """The reference's own fp32 evaluation (compute_dtype None) on the scene of `case`: the eight outputs and the four
    volume gradients for the upstream of _upstream()."""
    cfg, rm, vols, beta_v = scene(case)
    geo = PathGeometry(cfg)
    geom = torch.nan_to_num(O.frustum_to_ego(geo.frustum, None, None, None, None, prepared=rm), -1e3)
    beta = torch.tensor(beta_v) if cfg.density_mode == "sdf" else None
    v32 = [v.clone().requires_grad_(True) for v in vols]
    outs = O.render(geom, *v32, seg_bounds=(cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg),
                    output_coords=geo.output_coords, camera_mids=geo.camera_mids, bev_mids=geo.bev_mids,
                    d_far=cfg.d_bound[1], z_step_det=cfg.z_bound_det[2], num_classes=cfg.num_classes,
                    density_mode=cfg.density_mode, beta_param=beta, sdf_bias=cfg.sdf_bias, cat_seg=cfg.cat_seg)
    torch.autograd.backward(outs, _upstream([o.shape for o in outs], 4545, "cpu"))
    return [o.detach() for o in outs], [v.grad for v in v32]


@pytest.mark.parametrize("name", ["above-z-sdf", "outside-x", "oZ64", "narrow-4x200"])
def test_fp32_allowance_covers_the_reference_not_a_change(name):
    """The reference's own fp32 evaluation passes every output bar of out_err (fp32_allowance and the large-grid bars
    are no wider than its rounding needs), and voxel_density or bev_height scaled by 1.01 fails -- on the lattices in
    empty space as well, where both are 1e-4 - 1e-3 small."""
    case = CASE_BY_NAME[name]
    cfg = case.cfg
    ref = oracle_render(case)[0]
    got = fp32_reference(case)[0]
    bad = [f"{nm}: {e:.3e} > {b:.1e}" for nm, o in zip(NAMES, got) for e, b in [out_err(case, nm, o, ref)] if not e <= b]
    assert not bad, bad
    for nm in ("voxel_density", "bev_height_preds"):
        r = ref[NAMES.index(nm)]
        e, b = out_err(case, nm, r * 1.01, ref)
        assert e > b, (nm, e, b, float(r.abs().max()))


def test_sweep_reaches_every_bev_body():
    """Every BEV forward body (merged launch, one kernel, two kernels -- forced and on geometry), every backward body
    the shapes can reach (saved q-scan <21> / <0>, q kernel + scan, composited gather overwriting / accumulating, the
    cat_seg column gather with one and with several z segments, the pass-through gather, the generic gather, the zero
    path, the v1 splat) and both LDS regimes of both scans are reached by at least one case.  The composited column
    gather, the pass-through column gather and the <0> q-scan on 21 channels run above 2 GB tensors only: those are
    reached by big_descriptors(), whose plans test_library_plan_is_the_mirrors compares with the library's."""
    fwd, bodies, lds = set(), set(), set()
    for c in CASES:
        for path in PATHS:
            pl = plan(c, path)
            fwd.add((pl["fwd"], PATHS[path]["bev_fused"]))
            bodies |= pl["bodies"]
            if pl["lds"]:
                lds.add(pl["lds"])
            assert pl["comp_ok"] and pl["pass_ok"], c.name
    assert fwd == {("merged", True), ("fused", True), ("two-kernel", True), ("two-kernel", False)}, fwd
    assert bodies == {"qscan21", "qscan0", "q", "comp-overwrite", "comp-accumulate", "col-seg", "col-seg-zsegments",
                      "pass", "generic", "zero", "v1"}, sorted(bodies)
    assert lds == {(k, big) for k in ("q", "qscan") for big in (False, True)}, lds
    # the saved q-scan's one-wave-per-height split: below, at and above kQsMaxWaves heights
    ozs = {c.cfg.oZ for c in CASES}
    assert {1, QS_MAX_WAVES, QS_MAX_WAVES + 1, BEV_MAX_OZ} <= ozs
    assert any(plan(c)["qscan"] == 21 and plan(c)["qs_lds"] > LDS_RAISE for c in CASES)
    big = {name: lib_plan(d, ozs, flags) for name, d, ozs, flags in big_descriptors()}
    assert big["comp-col"]["comp_body"] == _capi.VAMP_BEVPLAN_BODY_COL and big["comp-col"]["pass_ok"]
    assert big["pass-col"]["base_body"] == _capi.VAMP_BEVPLAN_BODY_COL and big["pass-col"]["comp_ok"]
    assert big["qscan0-21ch"]["scan"] == _capi.VAMP_BEVPLAN_SCAN_QSCAN0 and big["qscan0-21ch"]["fits"]
    assert (big["offsets"], big["both-halves"], big["oZ65"]) == (ERR_OFFSETS, ERR_HALVES, ERR_HEIGHTS)


def test_library_agrees_with_the_mirrors():
    """The library's host-side answers on every case (f32 and bf16 descriptors): vamp_render_forward_merged_supported
    is the mirror's prediction, and vamp_render_bev_workspace_bytes covers what both scans write -- the non-saved
    scan's d beta partials included."""
    from vampire_amd.build import build_library
    build_library(verbose=False)
    lib = _capi.load()
    for c in CASES:
        for bf16 in (False, True):
            case = dataclasses.replace(c, bf16=bf16)
            d, ozs = desc(case), ozs_host(case)
            arr = (C.c_float * len(ozs))(*[float(v) for v in ozs])
            assert lib.vamp_render_forward_merged_supported(C.byref(d), arr) == int(merged_supported(d, ozs)), c.name
            got = lib.vamp_render_bev_workspace_bytes(C.byref(d))
            assert got == ws_needed(d), (c.name, got, ws_needed(d), scan_blocks(d, True), scan_blocks(d, False))


def library_plan(lib, d, ozs, flags):
    """vamp_render_bev_backward_plan's answer in lib_plan's form: the fields, or the refusal's message."""
    out = _capi.VampBevBackwardPlan()
    arr = None if ozs is None else (C.c_float * len(ozs))(*[float(v) for v in ozs])
    rc = lib.vamp_render_bev_backward_plan(C.byref(d), arr, flags, C.byref(out))
    if rc != 0:
        assert rc == -1, rc                       # VAMP_EINVAL
        msg = lib.vamp_last_error().decode()
        for known in (ERR_HEIGHTS, ERR_HALVES, ERR_OFFSETS):
            if msg.endswith("requirement failed: " + known):
                return known
        return msg
    return {n: list(getattr(out, n)) if isinstance(getattr(out, n), C.Array) else getattr(out, n) for n in PLAN_FIELDS}


def test_library_plan_is_the_mirrors():
    """vamp_render_bev_backward_plan -- the function vamp_render_bev_backward_ex asks before it launches -- answers
    what lib_plan predicts, field by field: every case x f32 / bf16 x SAVED_VALID x (OVERWRITE_BASE with and without
    OVERWRITE_CAM, no flags) x (whole call, SKIP_BASE, ONLY_BASE) x TABLE_VALID x host heights given / NULL; and on
    big_descriptors(): the column bodies of tensors above 2 GB, the <0> q-scan on 21 channels, and the three refusals.
    Every enumerator of the plan is met at least once."""
    from vampire_amd.build import build_library
    build_library(verbose=False)
    lib = _capi.load()
    A = _capi
    seen = {k: set() for k in ("path", "scan", "comp_body", "base_body", "base_body_no_vo", "beta_reduce",
                               "beta_reduce_no_vo", "table", "raise_lds", "outside", "generic", "seg_gather")}
    n = 0

    def check(what, d, ozs, flags):
        nonlocal n
        got, want = library_plan(lib, d, ozs, flags), lib_plan(d, ozs, flags)
        assert type(got) is type(want), (what, flags, got, want)
        if isinstance(want, dict):
            diff = {k: (got[k], want[k]) for k in PLAN_FIELDS if got[k] != want[k]}
            assert not diff, (what, flags, ozs is None, diff)
            for k in seen:
                seen[k].add(got[k])
        else:
            assert got == want, (what, flags, got, want)
        n += 1
        return got

    for c in CASES:
        for bf16 in (False, True):
            case = dataclasses.replace(c, bf16=bf16)
            d, ozs = desc(case), ozs_host(case)
            for saved in (0, A.VAMP_BEVBWD_SAVED_VALID):
                for ow in (A.VAMP_BEVBWD_OVERWRITE_BASE, A.VAMP_BEVBWD_OVERWRITE_BASE | A.VAMP_BEVBWD_OVERWRITE_CAM, 0):
                    for part in (0, A.VAMP_BEVBWD_SKIP_BASE, A.VAMP_BEVBWD_ONLY_BASE):
                        for tab in (0, A.VAMP_BEVBWD_TABLE_VALID):
                            for heights_given in (True, False):
                                check(c.name, d, ozs if heights_given else None, saved | ow | part | tab)
    assert n == len(CASES) * 2 * 2 * 3 * 3 * 2 * 2
    big = {name: check(name, d, ozs, flags) for name, d, ozs, flags in big_descriptors()}
    assert big["comp-col"]["comp_body"] == A.VAMP_BEVPLAN_BODY_COL and big["comp-col"]["comp_overwrite"] == 1
    assert big["pass-col"]["base_body"] == A.VAMP_BEVPLAN_BODY_COL and big["pass-col"]["base_overwrite"] == 1
    assert big["qscan0-21ch"]["scan"] == A.VAMP_BEVPLAN_SCAN_QSCAN0
    assert (big["offsets"], big["both-halves"], big["oZ65"]) == (ERR_OFFSETS, ERR_HALVES, ERR_HEIGHTS)
    assert seen["path"] == {A.VAMP_BEVPLAN_PATH_V1, A.VAMP_BEVPLAN_PATH_NOOP, A.VAMP_BEVPLAN_PATH_CELL}
    assert seen["scan"] == {A.VAMP_BEVPLAN_SCAN_NONE, A.VAMP_BEVPLAN_SCAN_QSCAN21, A.VAMP_BEVPLAN_SCAN_QSCAN0,
                            A.VAMP_BEVPLAN_SCAN_Q_SCAN}
    assert seen["comp_body"] == {A.VAMP_BEVPLAN_BODY_NONE, A.VAMP_BEVPLAN_BODY_COMP, A.VAMP_BEVPLAN_BODY_COL}
    assert seen["base_body"] == {A.VAMP_BEVPLAN_BODY_NONE, A.VAMP_BEVPLAN_BODY_PASS, A.VAMP_BEVPLAN_BODY_COL}
    assert seen["base_body_no_vo"] == {A.VAMP_BEVPLAN_BODY_NONE, A.VAMP_BEVPLAN_BODY_ZERO}
    assert seen["beta_reduce"] == {A.VAMP_BEVPLAN_BETA_NONE, A.VAMP_BEVPLAN_BETA_TAIL_COMP, A.VAMP_BEVPLAN_BETA_TAIL_BASE,
                                   A.VAMP_BEVPLAN_BETA_LAUNCH, A.VAMP_BEVPLAN_BETA_EARLY}
    assert seen["beta_reduce_no_vo"] == seen["beta_reduce"] - {A.VAMP_BEVPLAN_BETA_TAIL_BASE}
    assert all(seen[k] == {0, 1} for k in ("table", "raise_lds", "outside", "generic", "seg_gather"))
    # a NULL descriptor or plan is refused, not read
    assert lib.vamp_render_bev_backward_plan(None, None, 0, C.byref(_capi.VampBevBackwardPlan())) == -1
    assert lib.vamp_render_bev_backward_plan(C.byref(desc(Case("tiny"))), None, 0, None) == -1


# the C++ the mirrors above copy: if one of these lines changes, the mirror (and the reach table) needs a look
DISPATCH_SOURCE = {
    "render_common.hpp": [
        "const float per = fabsf(d->det_step[2]) * (float) (d->Z - 1) / d->span[2];",
        "return (int) ceilf((float) (d->oZ - 1) * per) + 4;",
        "const float g = ((pos - d->lo[2]) / d->span[2]) * 2.0f - 1.0f;",
        "const float f = ((g + 1.0f) / 2.0f) * (float) (d->Z - 1);",
        "return pmax - pmin + 2 <= bev_planes_alloc(d);"],
    "render_bev_fused.hip": [
        "return d->oZ <= kFusedMaxOZ && d->X >= 2 && (cmax > 3 ? cmax : 3) * V * es < 0x7fffffffull && "
        "omax < 0x7fffffffull && bev_planes_alloc(d) <= kFusedMaxNP;"],
    "render_bev_fused_dev.hpp": ["constexpr int kFusedMaxOZ = 64;", "constexpr int kFusedMaxNP = 40;"],
    "render_fwd_merged.hip": [
        "return d->D - 1 <= kPlanMax && bev_fwd_fused_supported(d) && d->oZ > 0 && d->oY > 0 && d->oX > 0;"],
    # (the backward's decisions are compared by value: test_library_plan_is_the_mirrors)
    "render_bev_dev.hpp": ["constexpr int kBevMaxOZ = 64;"],
    "render_bev.hip": ["constexpr int kQsMaxWaves = 16;", "constexpr int kMaxT = 3;", "#define VAMP_COLG 4"],
    "render_bev_fwd.hip": [
        "if (!(flags & VAMP_BEVFWD_TWO_KERNELS) && bev_fwd_fused_supported(d) && bev_fused_heights_fit(d, ozs_host))"],
}


def test_dispatch_mirrors():
    """The launcher lines the mirrors copy are still those of the source (DISPATCH_SOURCE): a change to the BEV dispatch
    fails here until the mirrors are brought along (the backward's dispatch is compared by value instead:
    test_library_plan_is_the_mirrors).  The mirrors at CFG_TINY: the one-kernel forward, the merged launch,
    three taps per axis, one z segment, the saved q-scan's <0> body."""
    from conftest import ROOT
    for fname, lines in DISPATCH_SOURCE.items():
        text = " ".join(open(os.path.join(ROOT, "vampire_amd", "csrc", fname)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, f"{fname}: dispatch line changed: {line}"
    from vampire_amd import ops
    assert ops.BEV_MAX_OZ == BEV_MAX_OZ
    tiny = plan(Case("tiny"))
    assert tiny["fwd"] == "merged" and tiny["preds"]["fused"] and tiny["fits"] and not tiny["zero"]
    assert tiny["nseg"] == 1 and tiny["qscan"] == 0
    assert Case("tiny").cfg.oZ == 2 and planes_alloc(desc(Case("tiny"))) == 5      # (int(2.4 / 0.8) == 2)
    assert plan(Case("K18", K=18))["qscan"] == 21
