"""The lift's workspace layout and plans (lift_common.hpp: lift_workspace; lift.hip: lift_forward_plan; lift_bwd_cell.hip:
lift_backward_plan), which the library answers on the host without a GPU.

The CPU tests hold the layout to the byte totals of the commit before it had one definition (PARENT_LAYOUT), compare
both plans with Python mirrors field by field and refusal by refusal over every descriptor x flag subset x workspace
size, check the refusals no sweep case reaches, and fail when a launcher line the mirrors copy changes.  The GPU test
shows that a backward the plan refuses has launched nothing: the workspace's cell counters are still what
VAMP_LIFTFWD_CELLS_CLEAN promises (about 1 s on an MI355X)."""
import ctypes as C
import dataclasses
import itertools
import os

import pytest
import torch

from conftest import ROOT
from vampire_amd import _capi
from vampire_amd.config import CFG_TINY, PRESETS
from vampire_amd.ops import lift_desc
from test_lift_bwd_cell_shapes import CASES as CELL_CASES
from test_render_shape_sweep import LIFT_DEPTHS, ask, depth_bound, library, subsets

A = _capi
ENOSPC, EINVAL = -2, -1
HUGE = 1 << 62

# ---------------------------------------------------------------------------------------------------- the descriptors
B = 2
TINY_CHANNELS = [4, 8, 16, 32, 64]
DEEP = 400                           # D whose strip gather needs more than 64 KB of LDS (raise_lds)


def named_cfgs():
    """(name, cfg, batch): every case of test_lift_bwd_cell_shapes at B = 2, the channel counts on CFG_TINY, the
    presets at batch 1 and 8, and -- for the softmax variants and the LDS limit -- the depths of the lift depth sweep
    and one deep descriptor."""
    for c in CELL_CASES:
        yield c.name, c.cfg, B
    for ch in TINY_CHANNELS:
        yield f"tiny-C{ch}", dataclasses.replace(CFG_TINY, mid_channels=ch), B
    for preset in "ABD":
        for batch in (1, 8):
            yield f"{preset}-b{batch}", PRESETS[preset], batch
    for D in LIFT_DEPTHS + [DEEP]:
        cfg = dataclasses.replace(CFG_TINY, d_bound=depth_bound(D - 1))
        assert cfg.D == D
        yield f"tiny-D{D}", cfg, B


def descs():
    """(name, descriptor): each configuration with and without depth, fp32 and bf16."""
    for name, cfg, batch in named_cfgs():
        for use_depth, dt in itertools.product((1, 0), (A.VAMP_F32, A.VAMP_BF16)):
            tag = f"{name}{'' if use_depth else '-nodepth'}{'-bf16' if dt == A.VAMP_BF16 else ''}"
            yield tag, name, lift_desc(cfg, batch, cfg.num_cams, cfg.mid_channels, dt, bool(use_depth))


# vamp_lift_workspace_bytes of the parent commit (LiftWs / carve in lift.hip around LiftCellWs / lift_cell_ws in
# lift_common.hpp), built on the CPU and asked once; the same for all four descriptors of a configuration (neither D nor
# in_dtype enters the layout)
PARENT_LAYOUT = {
    "grid-24x11x5": 1443584,
    "grid-72x3x2": 541184,
    "grid-16x16x5": 1402624,
    "cams-1": 479744,
    "cams-5": 2261760,
    "cams-9": 4027392,
    "C8": 1715968,
    "C16": 2342656,
    "C32": 3596032,
    "shared-cells": 1142528,
    "distinct-cells": 6224896,
    "fW16": 10471424,
    "fW24": 10512384,
    "fW22": 10506240,
    "D2": 1402624,
    "tiny-C4": 1402624,
    "tiny-C8": 1715968,
    "tiny-C16": 2342656,
    "tiny-C32": 3596032,
    "tiny-C64": 6102784,
    "A-b1": 1052563968,
    "A-b8": 8420474880,
    "B-b1": 518661376,
    "B-b8": 4149252608,
    "D-b1": 4112404224,
    "D-b8": 32899160064,
    "tiny-D2": 1402624,
    "tiny-D64": 1402624,
    "tiny-D65": 1402624,
    "tiny-D128": 1402624,
    "tiny-D129": 1402624,
    "tiny-D160": 1402624,
    "tiny-D400": 1402624,
}


def align_up(v, a=256):
    return (v + a - 1) // a * a


def ws_layout(d):
    """({region: (offset, bytes)}, total_bytes) of vamp_lift_workspace_layout."""
    out = A.VampLiftWorkspaceLayout()
    assert library().vamp_lift_workspace_layout(C.byref(d), C.byref(out)) == 0
    return {r: (out.offset[i], out.bytes[i]) for i, r in enumerate(A.LIFTWS_REGIONS)}, out.total_bytes


def test_workspace_layout_is_the_parents():
    """The byte query answers what the parent commit answered, the layout query agrees with it, and the regions are in
    the declared order, 256-byte aligned, non-empty and back to back; the cell lists begin behind the two feature
    copies, where the parent's `cells` block began."""
    lib = library()
    names = set()
    for tag, name, d in descs():
        total = lib.vamp_lift_workspace_bytes(C.byref(d))
        assert total == PARENT_LAYOUT[name], (tag, total, PARENT_LAYOUT[name])
        regions, layout_total = ws_layout(d)
        assert layout_total == total, (tag, layout_total, total)
        assert list(regions) == list(A.LIFTWS_REGIONS)
        assert all(off % 256 == 0 and nb % 256 == 0 and nb > 0 for off, nb in regions.values()), (tag, regions)
        at = 0
        for r in A.LIFTWS_REGIONS:
            assert regions[r][0] == at, (tag, r, regions[r], at)
            at += regions[r][1]
        assert at == total, (tag, at, total)
        assert regions["cnt"][0] == 2 * align_up(d.B * d.N * d.fH * d.fW * d.C * 4), (tag, regions["cnt"])
        names.add(name)
    assert names == set(PARENT_LAYOUT)
    some = next(descs())[2]
    assert lib.vamp_lift_workspace_layout(None, C.byref(A.VampLiftWorkspaceLayout())) == -1
    assert lib.vamp_lift_workspace_layout(C.byref(some), None) == -1


# ---------------------------------------------------------------------------------------------------- mirrors of the plans
SCAN_TILE = 2048                                       # common.hpp
TX = TY = 16                                           # lift_common.hpp: VAMP_LIFT_TX, VAMP_LIFT_TY
PIX, SPLIT, REG_BINS = 64, 4, 32                       # depth_softmax.hpp
KS, KW, KROW = 16, 4, 24                               # lift_bwd_cell.hip
FWD_FIELDS = [n for n, _ in A.VampLiftForwardPlan._fields_]
BWD_FIELDS = [n for n, _ in A.VampLiftBackwardPlan._fields_]
REQ = "requirement failed: "
ERR_CHANNELS = REQ + "C must be 4, 8 or a multiple of 16 (<= 64)"
ERR_FWD_FCL = REQ + "VAMP_LIFTFWD_FEAT_CHANNEL_LAST takes fp32 features (and depth)"
ERR_BWD_FCL = REQ + "VAMP_LIFTBWD_FEAT_CHANNEL_LAST takes fp32 features (and depth)"
ERR_LOGITS_DEPTH = REQ + "the logits entry is the depth-distribution lift"
ERR_LOGITS_F32 = REQ + "feat (and the depth distribution written here) are fp32"
ERR_LOGITS_DTYPE = REQ + "logits_dtype"
ERR_TILES = REQ + "too many tiles"
ERR_PAIRS = REQ + "pair / cell count exceeds 2^31"
ERR_CELL_COORDS = REQ + "feature map too large for the packed cell coordinates"
ERR_VOXELS = REQ + "voxel count exceeds 2^31"
ERR_SPLAT_LOGITS = REQ + "VAMP_LIFTBWD_LOGITS is a feature of the default (cell-list) backward"
ERR_CAMERAS = REQ + "at most 15 cameras (4-bit hit counters)"
ERR_LDS = ": D too large for the LDS depth tiles"


def validate(d):
    """lift.hip: lift_validate -- the first requirement the descriptor fails, or None."""
    checks = [(d.B > 0 and d.N > 0 and d.C > 0, "B, N, C must be positive"),
              (d.D > 0 and d.fH > 0 and d.fW > 0, "D, fH, fW must be positive"),
              (d.Z > 0 and d.Y > 0 and d.X > 0, "Z, Y, X must be positive"),
              (d.X < 32768 and d.Y < 32768 and d.fW < 32768 and d.fH < 32768, "axis too long for int16 taps"),
              (d.N <= 15, "at most 15 cameras (4-bit hit counters)"),
              (d.in_dtype in (A.VAMP_F32, A.VAMP_BF16), "in_dtype"),
              (d.use_depth == 1 or d.D == 1, "use_depth == 0 requires D == 1")]
    return next(((EINVAL, REQ + msg) for ok, msg in checks if not ok), None)


def channels_ok(ch):
    return ch in (4, 8) or (ch % 16 == 0 and ch <= 64)


def cells_fit(d):
    """lift_bwd_cell.hip: lift_cells_fit -- the shapes the cell lists cannot hold."""
    ncell = d.B * d.N * (d.fW + 1) * (d.fH + 1) + 2
    ncell = (ncell + SCAN_TILE - 1) // SCAN_TILE * SCAN_TILE
    if not (d.B * d.N * d.Z * d.Y * d.X < 2 ** 31 - 1 and ncell < 2 ** 31 - 1):
        return EINVAL, ERR_PAIRS
    if d.C % 4:
        return EINVAL, REQ + "C must be a multiple of 4"
    if not (d.fW < 32767 and d.fH < 32767 and d.D < 65535):
        return EINVAL, ERR_CELL_COORDS
    return None


def enospc(ws_bytes, need):
    return ENOSPC, f": workspace {ws_bytes} < {need} bytes"


def strip_lds_floats(D, cap):
    """lift_bwd_cell.hip: strip_lds_floats."""
    return D * KS * 2 + max(cap * KROW, KW * KS * 16, D * KS) + 2 * (KS + 2) + KS + 17 * KS + 8


def body(ch):
    return 4 if ch == 4 else (8 if ch == 8 else 16)


def fwd_plan(d, total, has_logits, logits_dtype, flags, ws_bytes):
    """lift.hip: lift_forward_plan -- the fields of VampLiftForwardPlan, or (code, message tail): the refusals in the
    order the library makes them."""
    bad = validate(d)
    if bad:
        return bad
    if has_logits:
        if d.use_depth != 1:
            return EINVAL, ERR_LOGITS_DEPTH
        if d.in_dtype != A.VAMP_F32:
            return EINVAL, ERR_LOGITS_F32
        if logits_dtype not in (A.VAMP_F32, A.VAMP_BF16):
            return EINVAL, ERR_LOGITS_DTYPE
    if not channels_ok(d.C):
        return EINVAL, ERR_CHANNELS
    fcl = bool(flags & A.VAMP_LIFTFWD_FEAT_CHANNEL_LAST)
    if fcl and d.in_dtype != A.VAMP_F32:
        return EINVAL, ERR_FWD_FCL
    p = dict.fromkeys(FWD_FIELDS, 0)
    p["bytes_needed"] = total
    BN, HW = d.B * d.N, d.fH * d.fW
    sm_tiles = (HW + PIX - 1) // PIX if has_logits else 0
    ptiles = 0 if fcl else (HW + 63) // 64
    if not BN * sm_tiles + BN * ptiles < 2 ** 31 - 1:
        return EINVAL, ERR_TILES
    p["first"] = ((A.VAMP_LIFTPLAN_FIRST_SOFTMAX if fcl else A.VAMP_LIFTPLAN_FIRST_OPERANDS) if has_logits else
                  (A.VAMP_LIFTPLAN_FIRST_NONE if fcl else A.VAMP_LIFTPLAN_FIRST_PROLOGUE))
    p.update(first_grid=BN * sm_tiles + BN * ptiles, sm_tiles=sm_tiles, ptiles=ptiles, cull_words=int(not fcl),
             sm_reg=int(bool(has_logits) and d.D <= SPLIT * REG_BINS), emit=int(bool(flags & A.VAMP_LIFTFWD_EMIT_PAIRS)))
    if p["emit"]:
        bad = cells_fit(d)
        if bad:
            return bad
        p["counters"] = (A.VAMP_LIFTPLAN_COUNTERS_CLEAN if flags & A.VAMP_LIFTFWD_CELLS_CLEAN
                         else A.VAMP_LIFTPLAN_COUNTERS_ZERO)
        p["scan"] = int(not flags & A.VAMP_LIFTFWD_DEFER_SCAN)
    p["coop"] = int(d.C == 16 and not p["emit"])
    p["ch"] = 0 if p["coop"] else body(d.C)
    p["grid"] = ((d.X + TX - 1) // TX, (d.Y + TY - 1) // TY, d.Z * d.B)
    return enospc(ws_bytes, total) if ws_bytes < total else p


def bwd_plan(d, total, flags, ws_bytes):
    """lift_bwd_cell.hip: lift_backward_plan -- the fields of VampLiftBackwardPlan, or (code, message tail)."""
    bad = validate(d)
    if bad:
        return bad
    if not channels_ok(d.C):
        return EINVAL, ERR_CHANNELS
    p = dict.fromkeys(BWD_FIELDS, 0)
    p["feat_cl"] = int(bool(flags & A.VAMP_LIFTBWD_FEAT_CHANNEL_LAST))
    if p["feat_cl"] and d.in_dtype != A.VAMP_F32:
        return EINVAL, ERR_BWD_FCL
    p["bytes_needed"] = total
    BN, HW = d.B * d.N, d.fH * d.fW
    if flags & A.VAMP_LIFTBWD_SPLAT:
        if flags & A.VAMP_LIFTBWD_LOGITS:
            return EINVAL, ERR_SPLAT_LOGITS
        p.update(path=A.VAMP_LIFTPLAN_BWD_SPLAT, to_cl=int(not p["feat_cl"]), to_cf=int(not p["feat_cl"]),
                 zero_feat_bytes=BN * HW * d.C * 4, zero_depth_bytes=BN * d.D * HW * 4 if d.use_depth else 0,
                 splat_ch=body(d.C), splat_grid=((d.X + TX - 1) // TX, (d.Y + TY - 1) // TY, d.Z * d.B))
        return enospc(ws_bytes, total) if ws_bytes < total else p
    p.update(path=A.VAMP_LIFTPLAN_BWD_CELL, prepare=int(not flags & A.VAMP_LIFTBWD_CELLS_VALID))
    if p["prepare"]:
        bad = cells_fit(d)
        if bad:
            return bad
    wps = (d.Z * d.Y * d.X + 63) // 64
    if not (wps * 64 < 2 ** 31 - 1 and wps * d.B < 2 ** 31 - 1):
        return EINVAL, ERR_VOXELS
    p.update(fill_ch=body(d.C), fill_grid=(wps * d.B + 3) // 4, fill_lds=4 * 64 * (2 + d.C // 4) * 16)
    p["cap"] = (128 if flags & A.VAMP_LIFTBWD_WPP1 else 64 if flags & A.VAMP_LIFTBWD_WPP4
                else 32 if flags & A.VAMP_LIFTBWD_WPP16 else 128)
    p["strip_lds"] = strip_lds_floats(d.D if d.use_depth else 0, p["cap"]) * 4
    if p["strip_lds"] > 150 * 1024:
        return EINVAL, ERR_LDS
    p.update(raise_lds=int(p["strip_lds"] > 64 * 1024), vec=int(d.in_dtype == A.VAMP_F32 and d.fW % 4 == 0),
             strip_grid=BN * d.fH * ((d.fW + KS - 1) // KS), softmax_bwd=int(bool(flags & A.VAMP_LIFTBWD_LOGITS)))
    return enospc(ws_bytes, total) if ws_bytes < total else p


def same_plan(got, want, what):
    """The library's answer `got` is the mirror's `want`: every field, or the refusal's code and message tail."""
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and got[0] == want[0] and got[1].endswith(want[1]), (what, got, want)
        return
    assert not isinstance(got, tuple), (what, got, want)
    have = {k: (list(v) if hasattr(v, "__len__") else v) for k, v in ((k, getattr(got, k)) for k in want)}
    norm = lambda k, v: list(v) if isinstance(v, (tuple, list)) else ([v] * len(have[k]) if isinstance(have[k], list) else v)
    diff = {k: (have[k], v) for k, v in want.items() if have[k] != norm(k, v)}     # (an array field left at 0: all zeros)
    assert not diff, (what, diff)


def fwd(d, has_logits=0, logits_dtype=0, flags=0, ws=HUGE):
    return ask(library().vamp_lift_forward_plan, A.VampLiftForwardPlan, C.byref(d), has_logits, logits_dtype, flags, ws)


def bwd(d, flags=0, ws=HUGE):
    return ask(library().vamp_lift_backward_plan, A.VampLiftBackwardPlan, C.byref(d), flags, ws)


def test_lift_plans_are_the_mirrors():
    """vamp_lift_forward_plan and vamp_lift_backward_plan -- the functions the entry points ask before their first
    launch -- answer what the mirrors predict, field by field and refusal by refusal: every descriptor x every subset
    of the flags x logits none / f32 / bf16 x a workspace one byte short and exact."""
    fwd_flags = subsets([A.VAMP_LIFTFWD_EMIT_PAIRS, A.VAMP_LIFTFWD_CELLS_CLEAN, A.VAMP_LIFTFWD_FEAT_CHANNEL_LAST,
                         A.VAMP_LIFTFWD_DEFER_SCAN])
    bwd_flags = subsets([A.VAMP_LIFTBWD_CELLS_VALID, A.VAMP_LIFTBWD_SPLAT, A.VAMP_LIFTBWD_WPP1, A.VAMP_LIFTBWD_WPP4,
                         A.VAMP_LIFTBWD_WPP16, A.VAMP_LIFTBWD_LOGITS, A.VAMP_LIFTBWD_FEAT_CHANNEL_LAST])
    assert len(fwd_flags) == 16 and len(bwd_flags) == 128
    seen = {k: set() for k in ("first", "coop", "body", "sm_reg", "counters", "scan", "path", "vec", "cap", "raise_lds",
                               "prepare", "refusal")}
    n = 0
    for tag, name, d in descs():
        total = library().vamp_lift_workspace_bytes(C.byref(d))
        for ws in (total - 1, total):
            for f in fwd_flags:
                for has_logits, ldt in ((0, 0), (1, A.VAMP_F32), (1, A.VAMP_BF16)):
                    want = fwd_plan(d, total, has_logits, ldt, f, ws)
                    same_plan(fwd(d, has_logits, ldt, f, ws), want, (tag, has_logits, ldt, f, ws))
                    n += 1
                    if isinstance(want, dict):
                        seen["first"].add(want["first"]), seen["coop"].add(want["coop"])
                        seen["counters"].add(want["counters"]), seen["scan"].add((want["emit"], want["scan"]))
                        if not want["coop"]:
                            seen["body"].add((want["ch"], want["emit"]))
                        if has_logits:
                            seen["sm_reg"].add(want["sm_reg"])
                    else:
                        seen["refusal"].add("ENOSPC" if want[0] == ENOSPC else want[1])
            for f in bwd_flags:
                want = bwd_plan(d, total, f, ws)
                same_plan(bwd(d, f, ws), want, (tag, f, ws))
                n += 1
                if isinstance(want, dict):
                    seen["path"].add(want["path"])
                    if want["path"] == A.VAMP_LIFTPLAN_BWD_CELL:
                        seen["vec"].add(want["vec"]), seen["cap"].add(want["cap"]), seen["prepare"].add(want["prepare"])
                        seen["raise_lds"].add(want["raise_lds"])
                else:
                    seen["refusal"].add("ENOSPC" if want[0] == ENOSPC else want[1])
    assert n == 4 * len(PARENT_LAYOUT) * 2 * (3 * len(fwd_flags) + len(bwd_flags)), n      # 46 464 answers
    assert seen["first"] == {0, 1, 2, 3} and seen["coop"] == {0, 1} and seen["sm_reg"] == {0, 1}
    assert seen["body"] == {(ch, e) for ch in (4, 8, 16) for e in (0, 1)}, seen["body"]
    assert seen["counters"] == {0, 1, 2} and seen["scan"] == {(0, 0), (1, 0), (1, 1)}
    assert seen["path"] == {0, 1} and seen["vec"] == {0, 1} and seen["cap"] == {128, 64, 32}
    assert seen["raise_lds"] == {0, 1} and seen["prepare"] == {0, 1}
    assert seen["refusal"] == {"ENOSPC", ERR_FWD_FCL, ERR_BWD_FCL, ERR_LOGITS_DEPTH, ERR_LOGITS_F32,
                               ERR_SPLAT_LOGITS}, seen["refusal"]
    # D on both sides of kSplit * kRegBins, and of the 64 KB above which the strip gather's LDS limit is raised
    depths = {d.D for _, _, d in descs()}
    assert {SPLIT * REG_BINS, SPLIT * REG_BINS + 1} <= depths
    assert strip_lds_floats(DEEP, 128) * 4 > 64 * 1024 > strip_lds_floats(max(LIFT_DEPTHS), 128) * 4


def test_lift_plan_refusals():
    """Each refusal no sweep case reaches, by code and message; what the same descriptor is allowed where the refusal
    does not apply; and a NULL descriptor or plan."""
    lib = library()
    tiny = lambda **kw: lift_desc(dataclasses.replace(CFG_TINY, **kw), 1, 6, kw.get("mid_channels", 4), A.VAMP_F32)
    EMIT, FCL = A.VAMP_LIFTFWD_EMIT_PAIRS, A.VAMP_LIFTFWD_FEAT_CHANNEL_LAST

    def refused(got, code, tail):
        assert isinstance(got, tuple) and got[0] == code and got[1].endswith(tail), (got, code, tail)

    def planned(got):
        assert not isinstance(got, tuple), got
        return got

    def mirrored(d, name):
        """(whatever the answer: the mirrors give it too)"""
        total = lib.vamp_lift_workspace_bytes(C.byref(d))
        for f in (0, EMIT, FCL, EMIT | FCL):
            for has_logits in (0, 1):
                same_plan(fwd(d, has_logits, 0, f), fwd_plan(d, total, has_logits, 0, f, HUGE), (name, has_logits, f))
        for f in (0, A.VAMP_LIFTBWD_CELLS_VALID, A.VAMP_LIFTBWD_SPLAT, A.VAMP_LIFTBWD_SPLAT | A.VAMP_LIFTBWD_LOGITS):
            same_plan(bwd(d, f), bwd_plan(d, total, f, HUGE), (name, f))

    # more than 2^31 (voxel, camera) pairs: where pairs are emitted or the prepare pass runs inside the call
    many = tiny()
    many.B, many.Z, many.Y, many.X = 8, 300, 3000, 3000                 # 1.3e11 pairs, 2.7e9 voxels per sample
    refused(fwd(many, flags=EMIT), EINVAL, "vamp_lift_forward_plan: " + ERR_PAIRS)
    refused(bwd(many), EINVAL, "vamp_lift_backward_plan: " + ERR_PAIRS)
    assert planned(fwd(many)).emit == 0
    refused(bwd(many, A.VAMP_LIFTBWD_CELLS_VALID), EINVAL, ERR_VOXELS)     # (the fill's own limit)
    many.Z = 6                                                          # 2.6e9 pairs, 5.4e7 voxels per sample
    refused(bwd(many), EINVAL, ERR_PAIRS)
    assert planned(bwd(many, A.VAMP_LIFTBWD_CELLS_VALID)).prepare == 0
    mirrored(many, "many")
    # fW = 32767: one more than the packed cell coordinates hold, allowed where no cells are built
    wide = tiny()
    wide.fW = 32767
    refused(fwd(wide, flags=EMIT), EINVAL, ERR_CELL_COORDS)
    refused(bwd(wide), EINVAL, ERR_CELL_COORDS)
    assert planned(fwd(wide)).ptiles == (8 * 32767 + 63) // 64
    assert planned(bwd(wide, A.VAMP_LIFTBWD_CELLS_VALID)).strip_grid == 6 * 8 * 2048
    wide.fW = 32766
    assert planned(fwd(wide, flags=EMIT)).emit == 1
    wide.fW = 32768
    refused(fwd(wide), EINVAL, REQ + "axis too long for int16 taps")
    wide.fW = 32767
    mirrored(wide, "wide")
    # 16 cameras, 12 channels
    cams = tiny()
    cams.N = 16
    refused(fwd(cams), EINVAL, ERR_CAMERAS)
    refused(bwd(cams), EINVAL, ERR_CAMERAS)
    mirrored(cams, "cams")
    c12 = tiny()
    c12.C = 12
    refused(fwd(c12), EINVAL, "vamp_lift_forward_plan: " + ERR_CHANNELS)
    refused(bwd(c12, A.VAMP_LIFTBWD_SPLAT), EINVAL, "vamp_lift_backward_plan: " + ERR_CHANNELS)
    mirrored(c12, "C12")
    # flags that exclude each other
    refused(bwd(tiny(), A.VAMP_LIFTBWD_LOGITS | A.VAMP_LIFTBWD_SPLAT), EINVAL, ERR_SPLAT_LOGITS)
    half = tiny()
    half.in_dtype = A.VAMP_BF16
    refused(fwd(half, flags=FCL), EINVAL, ERR_FWD_FCL)
    refused(bwd(half, A.VAMP_LIFTBWD_FEAT_CHANNEL_LAST), EINVAL, ERR_BWD_FCL)
    refused(fwd(half, 1, A.VAMP_F32), EINVAL, ERR_LOGITS_F32)
    refused(fwd(tiny(), 1, A.VAMP_F16), EINVAL, ERR_LOGITS_DTYPE)
    flat = lift_desc(CFG_TINY, 1, 6, 4, A.VAMP_F32, use_depth=False)
    refused(fwd(flat, 1, A.VAMP_F32), EINVAL, ERR_LOGITS_DEPTH)
    # more tiles than a grid index: 16 x 15 images of 32767 x 32767 pixels
    tiles = tiny()
    tiles.B, tiles.N, tiles.fH, tiles.fW = 16, 15, 32767, 32767
    refused(fwd(tiles), EINVAL, ERR_TILES)
    assert planned(fwd(tiles, flags=FCL)).first == A.VAMP_LIFTPLAN_FIRST_NONE
    # the strip gather's LDS limit: the smallest refused D from the mirror
    deep_d = smallest_refused_depth()
    assert deep_d == 794                                                # 48 D + 332 > 38400 floats
    deep = lift_desc(dataclasses.replace(CFG_TINY, d_bound=(2.0, 2.0 + deep_d * 0.0625, 0.0625)), 1, 6, 4, A.VAMP_F32)
    assert deep.D == deep_d
    refused(bwd(deep), EINVAL, "vamp_lift_backward_plan" + ERR_LDS)
    refused(bwd(deep, A.VAMP_LIFTBWD_CELLS_VALID), EINVAL, ERR_LDS)
    assert planned(bwd(deep, A.VAMP_LIFTBWD_SPLAT)).path == A.VAMP_LIFTPLAN_BWD_SPLAT
    assert planned(fwd(deep, flags=EMIT)).emit == 1
    mirrored(deep, "deep")
    deep.D -= 1
    ok = planned(bwd(deep))
    assert ok.raise_lds == 1 and ok.strip_lds == strip_lds_floats(deep_d - 1, 128) * 4 <= 150 * 1024
    mirrored(deep, "deep - 1")
    # ENOSPC by name, and a NULL workspace counts as no bytes at the entry points (nothing is launched: no GPU needed)
    total = lib.vamp_lift_workspace_bytes(C.byref(tiny()))
    refused(fwd(tiny(), ws=total - 1), ENOSPC, f"vamp_lift_forward_plan: workspace {total - 1} < {total} bytes")
    refused(bwd(tiny(), ws=total - 1), ENOSPC, f"vamp_lift_backward_plan: workspace {total - 1} < {total} bytes")
    assert lib.vamp_lift_finish_cells(C.byref(tiny()), None, total, None) == ENOSPC
    assert lib.vamp_last_error().decode().endswith(f"vamp_lift_finish_cells: workspace 0 < {total} bytes")
    # a NULL descriptor or plan is refused, not read
    assert lib.vamp_lift_forward_plan(None, 0, 0, 0, 0, C.byref(A.VampLiftForwardPlan())) == EINVAL
    assert lib.vamp_last_error().decode().endswith("desc is NULL")
    assert lib.vamp_lift_forward_plan(C.byref(tiny()), 0, 0, 0, 0, None) == EINVAL
    assert lib.vamp_last_error().decode().endswith("plan is NULL")
    assert lib.vamp_lift_backward_plan(None, 0, 0, C.byref(A.VampLiftBackwardPlan())) == EINVAL
    assert lib.vamp_last_error().decode().endswith("desc is NULL")
    assert lib.vamp_lift_backward_plan(C.byref(tiny()), 0, 0, None) == EINVAL
    assert lib.vamp_last_error().decode().endswith("plan is NULL")


def smallest_refused_depth():
    """The smallest D whose strip gather does not fit the 150 KB of LDS a workgroup may ask for (default chunk)."""
    return next(D for D in range(1, 65535) if strip_lds_floats(D, 128) * 4 > 150 * 1024)


# the C++ the mirrors above copy: if one of these lines changes, the mirror needs a look
DISPATCH_SOURCE = {
    "lift.hip": ["p.sm_reg = has_logits && d->D <= kSplit * kRegBins;",
                 "const long sm_tiles = has_logits ? (HW + kPix - 1) / kPix : 0, ptiles = fcl ? 0 : (HW + 63) / 64;",
                 "p.coop = d->C == 16 && VAMP_LIFT_TX == 16 && VAMP_LIFT_TY == 16 && VAMP_LIFT_COOP && !p.emit;",
                 "p.ch = p.coop ? 0 : (d->C == 4 ? 4 : (d->C == 8 ? 8 : 16));",
                 "if (p.ch == 4) VAMP_FWD(4, true); else if (p.ch == 8) VAMP_FWD(8, true); else VAMP_FWD(16, true);",
                 "if (p.ch == 4) VAMP_FWD(4, false); else if (p.ch == 8) VAMP_FWD(8, false); else VAMP_FWD(16, false);",
                 "if (p.splat_ch == 4) VAMP_SPLAT(4); else if (p.splat_ch == 8) VAMP_SPLAT(8); else VAMP_SPLAT(16);",
                 "#define VAMP_LIFT_COOP 1"],
    "lift_bwd_cell.hip": ["constexpr int kS = 16;", "constexpr int kW = 4;", "constexpr int kRow = 24;",
                          "return (size_t) D * kS * 2 + (size_t) std::max(std::max(cap * kRow, kW * kS * 16), D * kS) "
                          "+ 2 * (kS + 2) + kS + 17 * kS + 8;",
                          "const int ch = d->C == 4 ? 4 : (d->C == 8 ? 8 : 16);",
                          "p.cap = (flags & VAMP_LIFTBWD_WPP1) ? 128 : ((flags & VAMP_LIFTBWD_WPP4) ? 64 : "
                          "((flags & VAMP_LIFTBWD_WPP16) ? 32 : 128));",
                          "if (p.strip_lds > 150 * 1024)", "p.raise_lds = p.strip_lds > 64 * 1024;",
                          "p.vec = d->in_dtype == VAMP_F32 && d->fW % 4 == 0;",
                          "if (p.fill_ch == 4) VAMP_CELL(4); else if (p.fill_ch == 8) VAMP_CELL(8); else VAMP_CELL(16);"],
    "lift_common.hpp": ["#define VAMP_LIFT_TX 16", "#define VAMP_LIFT_TY 16",
                        "inline bool lift_channels_ok(int C) { return C == 4 || C == 8 || (C % 16 == 0 && C <= 64); }"],
    "depth_softmax.hpp": ["constexpr int kPix = 64;", "constexpr int kSplit = 4;", "constexpr int kRegBins = 32;"],
    "common.hpp": ["constexpr int kScanTile = 2048;"],
}


def test_dispatch_mirrors():
    """The launcher lines the mirrors copy are still those of the source (DISPATCH_SOURCE): a change to the dispatch
    fails here until the mirrors are brought along."""
    for fname, lines in DISPATCH_SOURCE.items():
        text = " ".join(open(os.path.join(ROOT, "vampire_amd", "csrc", fname)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, f"{fname}: dispatch line changed: {line}"
    assert [body(ch) for ch in TINY_CHANNELS] == [4, 8, 16, 16, 16]
    assert [channels_ok(ch) for ch in (4, 8, 12, 16, 48, 64, 80)] == [True, True, False, True, True, True, False]


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
def test_refused_backward_launches_nothing(tiny_common, dev):
    """A backward the plan refuses (D one above the strip gather's LDS limit) has launched nothing: afterwards the
    workspace's cell counters are still zero, as VAMP_LIFTFWD_CELLS_CLEAN promises -- checked by the library itself
    under vamp_debug_checks -- and the forward + backward that then run on that workspace give test_lift_backward_tiny's
    gradients.  (Before the plan the fill pass ran first, and left its cursors in the counters for good.)"""
    from test_hip_parity import close, hot
    g = tiny_common
    lib = library()
    deep_d = smallest_refused_depth()
    cfg = dataclasses.replace(CFG_TINY, d_bound=(2.0, 2.0 + deep_d * 0.0625, 0.0625))
    assert cfg.D == deep_d
    hp = hot(cfg, dev)
    lm = g["lift_mats"][:1].to(dev).contiguous()
    gen = torch.Generator().manual_seed(11)
    depth = torch.randn(1, cfg.num_cams, cfg.D, cfg.fH, cfg.fW, generator=gen).softmax(dim=2).to(dev).requires_grad_(True)
    feat = g["feat"][:1].to(dev).requires_grad_(True)
    out = hp.lift(depth, feat, lm)
    with pytest.raises(A.VampireHipError, match="D too large for the LDS depth tiles"):
        out.backward(g["g_lift"][:1].to(dev))
    # the same workspace, a CFG_TINY descriptor (the layout does not depend on D)
    ws = hp._ws["lift"]
    d = lift_desc(CFG_TINY, 1, CFG_TINY.num_cams, 4, A.VAMP_F32)
    assert lib.vamp_lift_workspace_bytes(C.byref(d)) <= ws.numel()
    dep, ft, gout = (g[k][:1].to(dev).contiguous() for k in ("depth", "feat", "g_lift"))
    vox = torch.empty(1, 4, CFG_TINY.vZ, CFG_TINY.vY, CFG_TINY.vX, device=dev)
    hits = torch.empty(1, CFG_TINY.vZ, CFG_TINY.vY, CFG_TINY.vX, 1, dtype=torch.int64, device=dev)
    gd, gf = torch.empty_like(dep), torch.empty_like(ft)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    geom = (ptr(lm), ptr(hp.xs), ptr(hp.ys), ptr(hp.zs))
    lib.vamp_debug_checks(1)
    try:
        rc = lib.vamp_lift_forward_ex(C.byref(d), *geom, ptr(dep), ptr(ft), ptr(vox), ptr(hits), ptr(ws), ws.numel(),
                                      A.VAMP_LIFTFWD_EMIT_PAIRS | A.VAMP_LIFTFWD_CELLS_CLEAN, None)
        assert rc == 0, lib.vamp_last_error().decode()
        rc = lib.vamp_lift_backward_ex(C.byref(d), *geom, ptr(dep), ptr(ft), ptr(gout), ptr(hits), ptr(gd), ptr(gf),
                                       ptr(ws), ws.numel(), A.VAMP_LIFTBWD_CELLS_VALID, None)
        assert rc == 0, lib.vamp_last_error().decode()
        torch.cuda.synchronize()
    finally:
        lib.vamp_debug_checks(0)
    close(vox, g["lift"][:1], atol=1e-5, what="lift")
    close(gd, g["grad_depth"][:1], atol=1e-5, rtol=1e-5, scale="max", what="grad_depth")
    close(gf, g["grad_feat"][:1], atol=1e-5, rtol=1e-5, scale="max", chan_dim=2, what="grad_feat")
