"""The camera render branch (one-kernel forward, planned march, merged launch, per-ray backward, cell-list scatter,
heavy-cell splat) across voxel grids, rigs, batches and cell loads, against the oracle evaluated in float64
(oracle/aten_oracle.py, compute_dtype): every output and every gradient, on each forced path of
tests/test_render_shape_sweep.py ("the sweep").

Every other small-shape float64 test of the camera branch has CFG_TINY's 16 x 16 x 5 voxels, six cameras, B = 2 and
8 x 22 rays per image: every heavy cell is one chunk, every ray tile has 4 - 8 active depth indices, X = 16 is one ragged
x-run, the cell scan has 2 tiles.  The cases here move one thing at a time from CFG_TINY (K = 5, C = 4, S = 20,
final_dim (32, 88) unless the case says otherwise; the det grid keeps CFG_TINY's bounds, so where the seg range does not
contain it the BEV outputs are partly those of empty space -- they stay in the comparison, the two branches share their
gradient buffers).  Rig, bda, volumes, upstream gradients and bars are the sweep's.  Two density regimes: "mixed" is the
sweep's scene (the low-x half of the density times 0.4), "empty" scales the whole density volume so that no ray
terminates and every path sorts exactly the inside samples, which the CPU test counts per cell.

test_scenes_have_the_properties_of_their_names (CPU) maps each scene through the oracle's render_tap_indices and
asserts what the case is named for: chunk counts of the heavy cells, heavy / light x-neighbours, active depth indices
per ray tile, x-runs, scan tiles, listed runs above the gather's grid, ray tiles below the grid's padding.  REACHED
ties every such class to the cases that reach it.

Two scenes beyond the issue's table, because the float64 gradients show that its own leave a gap
(test_items_carry_gradient): thin-2x160x65's x-runs from kGatherGrid up -- the gather's second items -- hold exact
zeros and it lists 2 930 runs, so dense-2x160x65-b3 lists 27 376 of 31 200 (second items in accumulate mode, HotPath's
own, and in overwrite mode, thousands of them with gradient); grid-72x3x2's third x-run holds 1e-9 of the largest
gradient, grid-72x3x2-empty's the largest.

Also here: the termination table holds S for every ray of the "empty" cases (early termination really is idle), the
gather's overwrite mode (runs == nullptr, which HotPath never sends) on the two cases with more x-runs than
kGatherGrid, and the lift FORWARD on the fifteen scenes of tests/test_lift_bwd_cell_shapes.py, which checks gradients
only.

Largest errors seen on an MI355X over all cases and paths, one run (relative to max |reference|; the sweep's bars: outputs
1e-5, gradients 2e-5, grad_beta 4e-6, lift 2e-5; -s prints each case's):
  rgb_preds 7.3e-6, depth_preds 6.9e-6, grad_beta 1.5e-6 (grid-72x3x2); bev_height_preds 7.8e-6 (scan-269);
  seg_logits_preds 1.06e-5 (above the bar: REF_ERR), bev_rgb_preds 8.2e-6, bev_seg_logits_preds 8.4e-6, voxel_density
  7.0e-6, voxel_output 7.9e-6, grad_density_feature 1.84e-5, grad_semantic_logits 1.08e-5, grad_base 3.9e-6, grad_rgb
  6.3e-6 (thin-2x160x65, whose reference evaluated in fp32 is off the float64 one by as much: 1.81e-5 on
  grad_density_feature); rgb_preds 1.50e-5, seg_logits_preds 1.20e-5 (dense-2x160x65-b3, REF_ERR), seg_logits_preds
  1.30e-5 (grid-72x3x2-empty, REF_ERR); overwrite mode 1.82e-5 / 1.07e-5 / 6.3e-6 (thin), 1.71e-5 / 1.42e-5 / 9.5e-6
  (dense); lift forward 7.7e-6 (distinct-cells).
Every case runs all seven paths (where the merged launch is not offered, NO_MERGED, "merged" and "two-launch" make the
same calls): the longest, grid-24x11x5 (the first, with the start-up), takes 1.1 s, coarse-2m-K28 0.27 s, scan-269
0.21 s.  The GPU tests of this file take about 4 s on an MI355X, the float64 oracle on the CPU included."""
import ctypes as C
import dataclasses
import functools
import os

import pytest
import torch

from oracle import aten_oracle as O
from vampire_amd import _capi
from vampire_amd.config import CFG_TINY
from vampire_amd.geometry import PathGeometry
from test_hip_parity import NAMES, hot, _upstream
from test_deep_tiles import _term
from test_bev_grid_sweep import bound
from test_render_shape_sweep import (GRAD_BAR, LIFT_BAR, OUT_BAR, PATHS, VOLS, _Calls, check_path, library,
                                     oracle_render, rel_err, run_path, scene)
import test_lift_bwd_cell_shapes as lift_shapes

F64 = torch.float64
PROJECT_BAR = 1e-4
TINY = CFG_TINY

# ---------------------------------------------------------------------------------------------------- the constants
CELL_HEAVY = 32           # kCellHeavy: a cell with more records is summed once per corner (cam_cell_splat_kernel)
SPLAT_CHUNK = 256         # VAMP_SPLAT_CHUNK: ... in ceil(n / 256) chunks of n / chunks records, the last with the rest
RUN_VOX = 32              # kRunVox: voxels of an x-run, the gather's item
GATHER_GRID = 20480       # VAMP_GATHER_GRID: workgroups of the gather at most
SCAN_TILE = 2048          # kScanTile: cells per workgroup of the scan's first level
SCAN_ROUND = 256          # tile totals per round of the scan's second level
PLAN_MAX = 128            # kPlanMax
PLAN_BALANCE = 4          # plan_share: fewer active depth indices are not dealt out
TERM_OPTICAL_DEPTH = 18.0  # kTermOpticalDepth
GRID_PAD = 8              # the ray kernels' grids are padded to a multiple of 8 tiles

CONSTANT_SOURCE = {
    "render_common.hpp": ["#define VAMP_CELL_HEAVY 32", "constexpr int kCellHeavy = VAMP_CELL_HEAVY;",
                          "constexpr int kRunVox = 32;", "constexpr float kTermOpticalDepth = 18.0f;"],
    "cam_lists.hpp": ["#define VAMP_SPLAT_CHUNK 256", "constexpr int kSplatChunk = VAMP_SPLAT_CHUNK;",
                      "__host__ __device__ inline int splat_chunks(int n) { return (n + kSplatChunk - 1) / kSplatChunk; }",
                      "#define VAMP_GATHER_GRID 20480", "constexpr int kGatherGrid = VAMP_GATHER_GRID;",
                      "const int nrec = st[k + 1] - st[k], nchunk = splat_chunks(nrec), len = nrec / nchunk;",
                      "const int ix0 = bx * kRunVox, span = min(kRunVox, P.X - ix0) + 1;"],
    "render_bwd_cell.hip": ["const int nchunk = splat_chunks(cl.own_n), len = cl.own_n / nchunk;",
                            "const int* runs = accumulate ? w.runs : nullptr;",
                            "*gather_grid = (int) std::min<long>(a.total_runs, kGatherGrid);"],
    "common.hpp": ["constexpr int kScanTile = 2048;"],
    "runtime.hip": ["for (int b0 = 0; b0 < ntile; b0 += 256) {"],
    "ray_plan.hpp": ["constexpr int kPlanMax = 128;", "if (A < 4) {"],
}


def splat_chunks(n):
    return (n + SPLAT_CHUNK - 1) // SPLAT_CHUNK


# ---------------------------------------------------------------------------------------------------- the cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    x: tuple = TINY.x_bound_seg
    y: tuple = TINY.y_bound_seg
    z: tuple = TINY.z_bound_seg
    grid: tuple = (16, 16, 5)            # (X, Y, Z) the bounds must give
    N: int = 6
    B: int = 2
    K: int = 5
    final_dim: tuple = TINY.final_dim
    empty: float = None                  # None: "mixed"; a factor: the whole density volume times it ("empty")
    S: int = 20                          # (what the sweep's run_path / check_path read of a case)
    bf16: bool = False

    @property
    def cfg(self):
        cfg = dataclasses.replace(TINY, density_mode="sdf", x_bound_seg=self.x, y_bound_seg=self.y, z_bound_seg=self.z,
                                  num_cams=self.N, num_classes=self.K, final_dim=self.final_dim)
        assert (cfg.vX, cfg.vY, cfg.vZ) == self.grid and cfg.D - 1 == self.S, (self.name, cfg.vX, cfg.vY, cfg.vZ, cfg.D)
        return cfg


# (the largest optical depth of a ray in float64: 1.09 at grid-2x2x2 with the factor 0.4; on the 2 m voxels 0.4 gives
# 12.3, 0.35 4.9, 0.3 1.4 -- against the 18 at which a ray terminates)
COARSE = dict(x=bound(-16.0, 16, 2.0), y=bound(-16.0, 16, 2.0), z=bound(-2.0, 3, 2.0), grid=(16, 16, 3),
              final_dim=(64, 176), empty=0.3)

CASES = [
    Case("grid-24x11x5", x=(-6.0, 6.0, 0.5), y=(-2.75, 2.75, 0.5), grid=(24, 11, 5)),
    Case("grid-72x3x2", x=(-9.0, 9.0, 0.25), y=(-0.75, 0.75, 0.5), z=(-0.5, 1.5, 1.0), grid=(72, 3, 2)),
    Case("grid-33", x=bound(-6.4, 33, 12.8 / 33), grid=(33, 16, 5)),
    Case("grid-32", x=bound(-6.4, 32, 0.4), grid=(32, 16, 5)),
    Case("grid-2x2x2", x=bound(-6.4, 2, 6.4), y=bound(-6.4, 2, 6.4), z=bound(-2.0, 2, 2.0), grid=(2, 2, 2), empty=0.4),
    Case("tall-z40", z=bound(-2.0, 40, 0.8), grid=(16, 16, 40)),
    Case("offside", x=bound(3.2, 16, 0.8)),
    Case("slab-x2", x=bound(5.0, 2, 0.8), grid=(2, 16, 5)),
    Case("coarse-2m", **COARSE),
    Case("coarse-2m-K18", K=18, **COARSE),
    Case("coarse-2m-K28", K=28, **COARSE),
    Case("scan-269", x=bound(-6.4, 64, 0.2), y=bound(-6.4, 64, 0.2), z=bound(-2.0, 64, 0.0625), grid=(64, 64, 64)),
    Case("thin-2x160x65", x=bound(-0.8, 2, 0.8), y=bound(-8.0, 160, 0.1), z=bound(-2.0, 65, 0.1), grid=(2, 160, 65)),
    Case("cams1-b1", N=1, B=1),
    Case("cams7-b3", N=7, B=3),
    Case("img-4x6", final_dim=(16, 24)),
    # ---- beyond the issue's table: scenes with weight where the two above have none (test_items_carry_gradient)
    # grid-72x3x2 in the "empty" regime: its third x-run holds the tensors' largest gradients (mixed: 1e-9 of them)
    Case("grid-72x3x2-empty", x=(-9.0, 9.0, 0.25), y=(-0.75, 0.75, 0.5), z=(-0.5, 1.5, 1.0), grid=(72, 3, 2), empty=0.4),
    # 31 200 x-runs of which 27 376 hold records: the gather takes second items in accumulate mode too (thin lists
    # 2 930), and in overwrite mode the second items are runs of b = 1, 2 that rays cross (thin's hold exact zeros)
    Case("dense-2x160x65-b3", x=bound(-6.4, 2, 6.4), y=bound(-6.4, 160, 0.08), z=bound(-0.5, 65, 3.0 / 65),
         grid=(2, 160, 65), B=3, final_dim=(64, 176), empty=0.4),
]
CASE_BY_NAME = {c.name: c for c in CASES}
NO_MERGED = {"scan-269", "thin-2x160x65", "dense-2x160x65-b3"}    # the merged launch is not offered (test_library_plans_of_the_cases): two launches

# fp32 reference (the oracle with compute_dtype None, autograd for the gradients) against the float64 oracle, on the
# CPU: recorded where a case exceeds a bar of the sweep and the reference's own fp32 evaluation is within a factor two
# of the kernels' error -- that (case, tensor) gets twice this, never above the project's 1e-4.
# thin-2x160x65: Y = 160 and Z = 65 planes put 2^-24 (n - 1) = 9.5e-6 and 3.8e-6 of a voxel into the fp32 tap
# coordinate, which the kernels form as the reference does; every path gives 1.05e-5 - 1.06e-5 there.
# dense-2x160x65-b3 has the same grid (every path: rgb_preds 1.47e-5 - 1.50e-5, seg_logits_preds 1.20e-5); on
# grid-72x3x2-empty (X = 72 over 18 m) the planned march gives the reference's 1.16e-5, the one-kernel forward 1.30e-5.
REF_ERR = {("thin-2x160x65", "seg_logits_preds"): 1.051e-05,
           ("dense-2x160x65-b3", "rgb_preds"): 1.472e-05,
           ("dense-2x160x65-b3", "seg_logits_preds"): 1.205e-05,
           ("grid-72x3x2-empty", "seg_logits_preds"): 1.162e-05}


def bar_of(case, what, sweep_bar):
    """The sweep's bar, or twice the recorded error of the reference's own fp32 evaluation where that is larger."""
    key = (case.name, what.replace("no-grad ", "").replace("train ", ""))
    if key not in REF_ERR:
        return sweep_bar
    return min(max(sweep_bar, 2.0 * REF_ERR[key]), PROJECT_BAR)


# ---------------------------------------------------------------------------------------------------- the scenes' properties
def seg_bounds(cfg):
    return (cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg)


@functools.lru_cache(maxsize=None)
def samples(case):
    """(geom [B, N, D, fH, fW, 3], inside [B, N, S, fH, fW], cell [B, N, S, fH, fW]: the cell of each sample's floor
    taps, as the cell lists number them)."""
    cfg, rm = scene(case)[:2]
    X, Y, Z = case.grid
    geom = torch.nan_to_num(O.frustum_to_ego(PathGeometry(cfg).frustum, None, None, None, None, prepared=rm), -1e3)
    inside, ix0, iy0, iz0 = O.render_tap_indices(geom, seg_bounds(cfg), (Z, Y, X))
    ncell_b = (Z + 1) * (Y + 1) * (X + 1)
    b = torch.arange(case.B).view(-1, 1, 1, 1, 1)
    cell = b * ncell_b + ((iz0.long() + 1) * (Y + 1) + iy0.long() + 1) * (X + 1) + ix0.long() + 1
    return geom, inside, cell


def optical_depth(case):
    """The largest per-ray optical depth sum_i sigma_i delta_i of the camera branch, the sampling and the density in
    float64 (what the float64 oracle composites)."""
    cfg, rm, vols, beta_v = scene(case)
    geom, inside, _ = samples(case)
    B, N, D, H, W, _ = geom.shape
    lo = torch.tensor([b[0] for b in seg_bounds(cfg)])
    span = torch.tensor([b[1] - b[0] for b in seg_bounds(cfg)])
    g = ((geom[:, :, :-1] - lo) / span) * 2.0 - 1.0
    s = torch.nn.functional.grid_sample(vols[0].double(), g.double().reshape(B, -1, H, W, 3), align_corners=True)
    s = torch.nan_to_num(s.reshape(B, N, D - 1, H, W) * inside)
    sigma = O.density_sdf(s, torch.tensor(beta_v, dtype=F64), cfg.sdf_bias)
    delta = torch.norm(geom[:, :, 1:] - geom[:, :, :-1], dim=-1).double()
    return float((sigma * delta).sum(dim=2).max())


@functools.lru_cache(maxsize=None)
def stats(case):
    """What the kernels' code paths depend on, from the scene's inside samples (all of them: the "empty" regime)."""
    cfg = case.cfg
    X, Y, Z = case.grid
    _, inside, cell = samples(case)
    ncell = case.B * (Z + 1) * (Y + 1) * (X + 1)
    flat = torch.bincount(cell[inside], minlength=ncell)
    cnt = flat.view(case.B, Z + 1, Y + 1, X + 1)
    heavy = flat[flat > CELL_HEAVY]
    s = dict(records=int(flat.sum()), nmax=int(flat.max()), heavy=heavy.tolist(),
             chunks={splat_chunks(n) for n in heavy.tolist()})
    # x-neighbour cells share a range of the gather (cell_ranges_light): a heavy cell in front of a light one, and behind
    a, b = cnt[..., :-1], cnt[..., 1:]
    s["heavy_light"] = int(((a > CELL_HEAVY) & (b > 0) & (b <= CELL_HEAVY)).sum())
    s["light_heavy"] = int(((a > 0) & (a <= CELL_HEAVY) & (b > CELL_HEAVY)).sum())
    # a ray tile's active depth indices: those at which any ray of the 8 x 8 tile is inside the volume
    fH, fW = cfg.fH, cfg.fW
    th, tw = (fH + 7) // 8, (fW + 7) // 8
    pad = torch.nn.functional.pad(inside, (0, tw * 8 - fW, 0, th * 8 - fH))
    act = pad.view(case.B, case.N, case.S, th, 8, tw, 8).any(dim=6).any(dim=4).sum(dim=2).flatten()
    s["ray_tiles"] = act.numel()
    assert act.numel() == case.B * case.N * th * tw
    s["tiles_0"], s["tiles_1_3"], s["tiles_4"] = int((act == 0).sum()), int(((act >= 1) & (act < PLAN_BALANCE)).sum()), int((act >= PLAN_BALANCE).sum())
    # x-runs (cam_lists.hpp): run bx of row (b, iz, iy) is listed when the cells in reach of its voxels hold a record
    s["runs_x"] = runs_x = (X + RUN_VOX - 1) // RUN_VOX
    s["last_run"] = X - RUN_VOX * (runs_x - 1)
    s["total_runs"] = runs_x * Y * Z * case.B
    listed = 0
    for bx in range(runs_x):
        ix0 = bx * RUN_VOX
        span = min(RUN_VOX, X - ix0) + 1
        seg = cnt[..., ix0:ix0 + span].sum(dim=-1)                           # [B, Z + 1, Y + 1]
        listed += int(((seg[:, :-1, :-1] + seg[:, :-1, 1:] + seg[:, 1:, :-1] + seg[:, 1:, 1:]) > 0).sum())
    s["runs_listed"] = listed
    s["max_span"] = min(RUN_VOX, X) + 1
    # the scan: tiles of 2 048 cells, their totals scanned 256 per round
    s["scan_tiles"] = (ncell + 2 + SCAN_TILE - 1) // SCAN_TILE
    tile_of = torch.arange(ncell) // SCAN_TILE
    s["records_round_1"] = int(flat[tile_of >= SCAN_ROUND].sum())
    s["record_tiles_round_1"] = int((torch.bincount(tile_of[flat > 0], minlength=1)[SCAN_ROUND:] > 0).sum())
    s["records_round_0"] = int(flat[tile_of < SCAN_ROUND].sum())
    return s


def ragged_chunk(n):
    """A heavy cell whose chunks are no whole number of the splat's 32-record rounds, and whose last chunk is longer."""
    k = splat_chunks(n)
    return k >= 2 and (n // k) % 32 != 0 and n % k != 0


# what each case is named for, as predicates of stats(case)
WANT = {
    "grid-24x11x5": [("ray tiles with 1 - 3 active indices", lambda s: s["tiles_1_3"] >= 8)],
    "grid-72x3x2": [("three x-runs, the last of 8 voxels", lambda s: (s["runs_x"], s["last_run"]) == (3, 8)),
                    ("ray tiles with no active index", lambda s: s["tiles_0"] >= 8),
                    ("ray tiles with 1 - 3 active indices", lambda s: s["tiles_1_3"] >= 2)],
    "grid-33": [("two x-runs, the last of one voxel", lambda s: (s["runs_x"], s["last_run"]) == (2, 1))],
    "grid-32": [("one full x-run of 33 cells", lambda s: (s["runs_x"], s["last_run"], s["max_span"]) == (1, 32, 33))],
    "grid-2x2x2": [("two cells hold every record, in 16 chunks or more each",
                    lambda s: len(s["heavy"]) == 2 and sum(s["heavy"]) == s["records"] and min(s["heavy"]) > 16 * SPLAT_CHUNK),
                   ("their chunks are ragged", lambda s: all(ragged_chunk(n) for n in s["heavy"])),
                   ("one scan tile", lambda s: s["scan_tiles"] == 1)],
    "tall-z40": [("most x-runs hold no record", lambda s: s["total_runs"] == 1280 and 0 < s["runs_listed"] < s["total_runs"] // 2)],
    "offside": [("ray tiles with no active index", lambda s: s["tiles_0"] >= 8),
                ("ray tiles with 1 - 3 active indices", lambda s: s["tiles_1_3"] >= 1),
                ("a heavy cell in front of a light x-neighbour", lambda s: s["heavy_light"] >= 1)],
    "slab-x2": [("ray tiles with no active index", lambda s: s["tiles_0"] >= 8),
                ("ray tiles with 1 - 3 active indices", lambda s: s["tiles_1_3"] >= 4)],
    "coarse-2m": [("hundreds of one-chunk heavy cells", lambda s: sum(1 for n in s["heavy"] if n <= 256) >= 300),
                  ("cells of 257 - 512 records", lambda s: sum(1 for n in s["heavy"] if 257 <= n <= 512) >= 30),
                  ("cells of 513 - 768 records", lambda s: sum(1 for n in s["heavy"] if 513 <= n <= 768) >= 1),
                  ("a cell above 768 records", lambda s: s["nmax"] > 768),
                  ("ragged chunks", lambda s: sum(1 for n in s["heavy"] if ragged_chunk(n)) >= 10),
                  ("heavy-light and light-heavy x-neighbours", lambda s: s["heavy_light"] >= 10 and s["light_heavy"] >= 10)],
    "scan-269": [("269 scan tiles", lambda s: s["scan_tiles"] == 269),
                 ("records in several tiles of the second round", lambda s: s["records_round_1"] >= 100 and s["record_tiles_round_1"] >= 2),
                 ("records in the first round", lambda s: s["records_round_0"] >= 100)],
    "thin-2x160x65": [("more x-runs than the gather's grid", lambda s: s["total_runs"] == 20800 > GATHER_GRID)],
    "cams1-b1": [("fewer ray tiles than the grid's padding", lambda s: s["ray_tiles"] == 3 < GRID_PAD)],
    "cams7-b3": [("63 ray tiles", lambda s: s["ray_tiles"] == 63)],
    "img-4x6": [("one partial tile per camera", lambda s: s["ray_tiles"] == 12)],
}
WANT["coarse-2m-K18"] = WANT["coarse-2m-K28"] = WANT["coarse-2m"]
WANT["grid-72x3x2-empty"] = WANT["grid-72x3x2"][:1]
WANT["dense-2x160x65-b3"] = [("more x-runs with records than the gather's grid",
                              lambda s: s["total_runs"] == 31200 and s["runs_listed"] > GATHER_GRID + 4096)]

# every class of shape the camera branch's code distinguishes -> (predicate of (case, stats), the cases that reach it)
REACHED = {
    "heavy cells of one chunk": (lambda c, s: 1 in s["chunks"], {"coarse-2m", "grid-24x11x5"}),
    "heavy cells of two chunks": (lambda c, s: 2 in s["chunks"], {"coarse-2m"}),
    "heavy cells of three chunks": (lambda c, s: 3 in s["chunks"], {"coarse-2m"}),
    "heavy cells of four chunks or more": (lambda c, s: max(s["chunks"], default=0) >= 4, {"coarse-2m", "grid-2x2x2"}),
    "multi-chunk cells at CP 24": (lambda c, s: c.K == 18 and {2, 3} <= s["chunks"], {"coarse-2m-K18"}),
    "multi-chunk cells at CP 32": (lambda c, s: c.K == 28 and {2, 3} <= s["chunks"], {"coarse-2m-K28"}),
    "a chunk length that is no multiple of 32": (lambda c, s: any(ragged_chunk(n) for n in s["heavy"]), {"coarse-2m", "grid-2x2x2"}),
    "heavy-light x-neighbours": (lambda c, s: s["heavy_light"] > 0, {"coarse-2m", "offside"}),
    "light-heavy x-neighbours": (lambda c, s: s["light_heavy"] > 0, {"coarse-2m"}),
    "ray tiles with no active index": (lambda c, s: s["tiles_0"] > 0, {"grid-72x3x2", "offside", "slab-x2"}),
    "ray tiles with 1 - 3 active indices": (lambda c, s: s["tiles_1_3"] > 0, {"grid-24x11x5", "grid-72x3x2", "offside", "slab-x2"}),
    "ray tiles with 4 active indices or more": (lambda c, s: s["tiles_4"] > 0, {"grid-24x11x5", "cams7-b3"}),
    "one x-run": (lambda c, s: s["runs_x"] == 1, {"grid-24x11x5", "grid-32"}),
    "several x-runs": (lambda c, s: s["runs_x"] > 1, {"grid-72x3x2", "grid-33", "scan-269"}),
    "X a multiple of 32": (lambda c, s: c.grid[0] % RUN_VOX == 0, {"grid-32", "scan-269"}),
    "a last x-run of one voxel": (lambda c, s: s["runs_x"] > 1 and s["last_run"] == 1, {"grid-33"}),
    "X = 2": (lambda c, s: c.grid[0] == 2, {"grid-2x2x2", "slab-x2", "thin-2x160x65"}),
    "Z = 2": (lambda c, s: c.grid[2] == 2, {"grid-72x3x2", "grid-2x2x2"}),
    "one scan tile": (lambda c, s: s["scan_tiles"] == 1, {"grid-2x2x2"}),
    "more than 256 scan tiles, records beyond the first round": (
        lambda c, s: s["scan_tiles"] > SCAN_ROUND and s["records_round_1"] > 0, {"scan-269"}),
    "more x-runs than the gather's grid": (lambda c, s: s["total_runs"] > GATHER_GRID, {"thin-2x160x65", "dense-2x160x65-b3"}),
    "more x-runs with records than the gather's grid": (lambda c, s: s["runs_listed"] > GATHER_GRID, {"dense-2x160x65-b3"}),
    "x-runs without a record": (lambda c, s: s["runs_listed"] < s["total_runs"], {"tall-z40", "thin-2x160x65"}),
    "fewer than 8 ray tiles": (lambda c, s: s["ray_tiles"] < GRID_PAD, {"cams1-b1"}),
    "ray tiles no multiple of 8": (lambda c, s: s["ray_tiles"] % GRID_PAD != 0, {"cams1-b1", "cams7-b3"}),
    "an image smaller than a tile": (lambda c, s: c.cfg.fH < 8 and c.cfg.fW < 8, {"img-4x6"}),
    "N = 1": (lambda c, s: c.N == 1, {"cams1-b1"}),
    "N = 6": (lambda c, s: c.N == 6, {"grid-32"}),
    "N = 7": (lambda c, s: c.N == 7, {"cams7-b3"}),
    "B = 1": (lambda c, s: c.B == 1, {"cams1-b1"}),
    "B = 2": (lambda c, s: c.B == 2, {"grid-32"}),
    "B = 3": (lambda c, s: c.B == 3, {"cams7-b3"}),
}


def test_constants_are_the_kernels():
    """The constants the scenes are built around are still those of the source."""
    from conftest import ROOT
    for fname, lines in CONSTANT_SOURCE.items():
        text = " ".join(open(os.path.join(ROOT, "vampire_amd", "csrc", fname)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, f"{fname}: line changed: {line}"
    assert (CELL_HEAVY, SPLAT_CHUNK, RUN_VOX, GATHER_GRID, SCAN_TILE, PLAN_MAX) == (32, 256, 32, 20480, 2048, 128)
    assert all(c.S <= PLAN_MAX for c in CASES)                   # every case is planned: the ray plan's paths run


def test_scenes_have_the_properties_of_their_names():
    """Each scene has what its case is named for (WANT), each class of REACHED is reached by the cases it names, no ray
    of an "empty" case comes near termination in the float64 oracle, and CFG_TINY's own scene reaches none of the
    classes this file adds."""
    assert set(WANT) == {c.name for c in CASES}
    for c in CASES:
        s = stats(c)
        for what, ok in WANT[c.name]:
            assert ok(s), (c.name, what, {k: v for k, v in s.items() if k != "heavy"}, sorted(s["heavy"])[-8:])
        assert s["records"] > 0, c.name
        if c.empty is not None:
            tau = optical_depth(c)
            assert tau < TERM_OPTICAL_DEPTH / 2, (c.name, tau)
    for what, (ok, names) in REACHED.items():
        assert names, what
        for n in names:
            c = CASE_BY_NAME[n]
            assert ok(c, stats(c)), (what, n, {k: v for k, v in stats(c).items() if k != "heavy"})
    assert {c.name for c in CASES if c.empty is not None} == {"grid-2x2x2", "coarse-2m", "coarse-2m-K18", "coarse-2m-K28",
                                                              "grid-72x3x2-empty", "dense-2x160x65-b3"}
    # what the other small-shape tests have: one-chunk cells (63 records at most), 4 - 8 active indices, one ragged run
    t = stats(Case("tiny"))
    assert t["chunks"] == {1} and t["nmax"] < 2 * CELL_HEAVY and t["tiles_0"] == t["tiles_1_3"] == 0
    assert (t["runs_x"], t["last_run"], t["scan_tiles"], t["ray_tiles"]) == (1, 16, 2, 36)


VISIBLE = 100 * GRAD_BAR      # a gradient that large, relative to its tensor's largest, cannot go missing under GRAD_BAR


@functools.lru_cache(maxsize=None)
def run_weight(case):
    """[total_runs], in the gather's run order ((b Z + iz) Y + iy) runs_x + bx: the largest float64 camera-only
    gradient inside each x-run, relative to the largest of its tensor (the maximum over density, semantic and rgb)."""
    X = case.grid[0]
    runs_x = (X + RUN_VOX - 1) // RUN_VOX
    out = None
    for t in oracle_camera_only(case).values():
        a = t.abs().amax(dim=1) / t.abs().max()                                   # [B, Z, Y, X]
        a = torch.nn.functional.pad(a, (0, runs_x * RUN_VOX - X)).unflatten(-1, (runs_x, RUN_VOX)).amax(dim=-1)
        out = a if out is None else torch.maximum(out, a)
    return out.flatten()


def test_items_carry_gradient():
    """The x-runs a case is named for hold gradient that the comparison can see (VISIBLE, relative to the tensor's
    largest).  Second items of the gather: in overwrite mode item = run, so they are the runs from kGatherGrid up; in
    accumulate mode they are whatever the list holds beyond kGatherGrid entries, in the order of its atomics -- of
    dense-2x160x65-b3's listed runs more than kGatherGrid are visible, so any such tail holds thousands of them.
    thin-2x160x65 (the issue's case for the overwrite mode) has NO weight there: its runs from kGatherGrid up are
    z = 4.3 - 4.5 m of b = 1, which no ray crosses, and it lists 2 930 runs; alone it would pass a gather that drops
    its second items.  It checks the overwrite mode's stores of the first items and of zeros."""
    dense = CASE_BY_NAME["dense-2x160x65-b3"]
    w, s = run_weight(dense), stats(dense)
    assert w.numel() == s["total_runs"] and int((w > 0).sum()) == s["runs_listed"]
    assert int((w[GATHER_GRID:] > VISIBLE).sum()) > 4096                      # overwrite mode
    assert int((w > VISIBLE).sum()) > GATHER_GRID + 2048                      # accumulate mode: any tail of the list
    thin = run_weight(CASE_BY_NAME["thin-2x160x65"])
    assert float(thin[GATHER_GRID:].max()) == 0.0 and int((thin[:GATHER_GRID] > VISIBLE).sum()) > 1024
    # the last x-run of a row: grid-33's single voxel, scan-269's full second run, grid-72x3x2's third run of 8 -- in
    # the mixed regime that one holds 1e-9 of the largest gradient (the case checks its tiles and Z = 2, not that run)
    for name, last in (("grid-33", 1), ("scan-269", 1), ("grid-72x3x2-empty", 2)):
        c = CASE_BY_NAME[name]
        per_bx = run_weight(c).view(-1, stats(c)["runs_x"])
        assert per_bx.shape[1] == last + 1 and int((per_bx[:, last] > VISIBLE).sum()) >= 4, (name, float(per_bx[:, last].max()))
    mixed = run_weight(CASE_BY_NAME["grid-72x3x2"]).view(-1, 3)
    assert float(mixed[:, 2].max()) < GRAD_BAR and float(mixed[:, :2].max()) == 1.0


def test_library_plans_of_the_cases():
    """The library offers the merged launch on every case's descriptor and heights (check_path expects its calls) but
    NO_MERGED's, whose two det heights lie 26 of 64, 16 of 65 and 34 of 65 z planes apart: more than the BEV blocks' slab holds
    (they run the two launches on every path).  The backward's grids are those of the listed classes: min(total_runs, kGatherGrid)
    gather workgroups, ray tiles padded to 8, a list-building workgroup per scan tile and per 256 x-runs."""
    from vampire_amd.geometry import axis_centres
    from vampire_amd.ops import render_desc
    from test_bev_grid_sweep import f32, fused_supported, heights_fit
    lib = library()
    for c in CASES:
        cfg = c.cfg
        d = render_desc(cfg, c.B, c.N, _capi.VAMP_F32)
        ozs = axis_centres(cfg.z_bound_det).tolist()
        ok = lib.vamp_render_forward_merged_supported(C.byref(d), (C.c_float * len(ozs))(*ozs))
        assert ok == (0 if c.name in NO_MERGED else 1), c.name
        assert fused_supported(d) and heights_fit(d, [f32(v) for v in ozs]) == bool(ok), c.name
        p = _capi.VampCameraBackwardPlan()
        assert lib.vamp_render_camera_backward_plan(C.byref(d), 0, 1, _capi.VAMP_CAMBWD_ACCUMULATE, 0, 1 << 62, C.byref(p)) == 0
        s = stats(c)
        assert p.gather_grid == min(s["total_runs"], GATHER_GRID) and p.ray_grid == (s["ray_tiles"] + 7) // 8 * 8, c.name
        assert p.list_grid == s["scan_tiles"] + (s["total_runs"] + 255) // 256, c.name


@functools.lru_cache(maxsize=None)
def fp32_reference_errors(case):
    """{tensor: rel_err} of the reference's own fp32 evaluation (compute_dtype None, autograd for the gradients) against
    the float64 oracle, on the case's scene and the upstream of _upstream()."""
    cfg, rm, vols, beta_v = scene(case)
    ref_outs, ref_grads, _, _ = oracle_render(case)
    geo = PathGeometry(cfg)
    geom = torch.nan_to_num(O.frustum_to_ego(geo.frustum, None, None, None, None, prepared=rm), -1e3)
    v32 = [v.clone().requires_grad_(True) for v in vols]
    outs = O.render(geom, *v32, seg_bounds=seg_bounds(cfg), output_coords=geo.output_coords,
                    camera_mids=geo.camera_mids, bev_mids=geo.bev_mids, d_far=cfg.d_bound[1],
                    z_step_det=cfg.z_bound_det[2], num_classes=cfg.num_classes, density_mode="sdf",
                    beta_param=torch.tensor(beta_v), sdf_bias=cfg.sdf_bias, cat_seg=cfg.cat_seg)
    torch.autograd.backward(outs, _upstream([o.shape for o in outs], 4545, "cpu"))
    errs = {nm: rel_err(o, r) for nm, o, r in zip(NAMES, outs, ref_outs)}
    errs.update({f"grad_{k}": rel_err(v.grad, r) for k, v, r in zip(VOLS, v32, ref_grads)})
    return errs


def test_raised_bars_are_the_fp32_references():
    """Every bar above the sweep's is backed by REF_ERR, and REF_ERR by the reference's own fp32 evaluation: recomputed
    here it is what the table records (to a quarter: fp32 sums differ between CPUs), and it uses up more than half of
    the sweep's bar -- a tensor whose fp32 reference is far below the bar gets no allowance."""
    sweep = {**{nm: OUT_BAR for nm in NAMES}, **{f"grad_{k}": GRAD_BAR for k in VOLS}}
    for (name, what), recorded in REF_ERR.items():
        case = CASE_BY_NAME[name]
        got = fp32_reference_errors(case)[what]
        assert 0.75 * recorded <= got <= 1.25 * recorded, (name, what, got, recorded)
        assert 2.0 * recorded > sweep[what], (name, what, recorded)
        assert sweep[what] < bar_of(case, what, sweep[what]) <= min(2.0 * recorded, PROJECT_BAR)
    for c in CASES:
        for what, b in sweep.items():
            assert bar_of(c, what, b) == b or (c.name, what) in REF_ERR


# ---------------------------------------------------------------------------------------------------- GPU: render
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_camera_sweep_against_float64_oracle(dev, case):
    """Each forced path of the case: the eight outputs (no-grad and training forward), the four volume gradients and
    grad_beta against the float64 oracle; the C calls made are those of the path.  In the "empty" regime the merged
    no-grad forward leaves S in the termination table for every ray: early termination is idle, the cells hold the
    records the CPU test counted."""
    cfg = case.cfg
    hp = hot(cfg, dev)
    d = hp.render_desc(case.B, case.N, _capi.VAMP_F32)
    merged_ok = hp.lib.vamp_render_forward_merged_supported(C.byref(d), hp.ozs_host) == 1
    assert merged_ok == (case.name not in NO_MERGED)
    worst = {}
    bad = []
    for path in PATHS:
        errs, calls = run_path(case, path, dev)
        check_path(case, path, calls, merged_ok)
        for what, (e, b) in errs.items():
            b = bar_of(case, what, b)
            kind = what.replace("no-grad ", "").replace("train ", "")
            worst[kind] = max(worst.get(kind, 0.0), e)
            if not e <= b:
                bad.append(f"{path} {what}: {e:.3e} > {b:.1e}")
    print(f"\n{case.name}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    if case.empty is not None:
        _, rm, vols, beta_v = scene(case)
        hp = hot(cfg, dev)
        hp.impl.update(PATHS["merged"])
        with torch.no_grad():
            hp.render(*[v.to(dev) for v in vols], torch.tensor(beta_v, device=dev), render_mats=rm.to(dev))
        term = _term(hp, cfg, case.B).cpu()
        assert term.shape == (case.B * case.N, cfg.fH, cfg.fW)
        assert bool((term == case.S).all()), f"{case.name}: {int((term != case.S).sum())} rays terminate"
    assert not bad, f"{case.name}:\n" + "\n".join(bad)


class _Overwrite(_Calls):
    """The library with VAMP_CAMBWD_ACCUMULATE taken off every camera backward call (and the calls recorded as made)."""

    def __getattr__(self, name):
        call = _Calls.__getattr__(self, name)
        if name != "vamp_render_camera_backward_acc":
            return call

        def cleared(*a):
            a = list(a)
            a[-3] &= ~_capi.VAMP_CAMBWD_ACCUMULATE
            return call(*a)
        return cleared


@functools.lru_cache(maxsize=None)
def oracle_camera_only(case, seed=4545):
    """float64 oracle: the density, semantic and rgb gradients for the camera outputs' upstream of _upstream(), the
    BEV outputs' upstream zero."""
    cfg, rm, vols, beta_v = scene(case)
    geo = PathGeometry(cfg)
    geom = torch.nan_to_num(O.frustum_to_ego(geo.frustum, None, None, None, None, prepared=rm), -1e3)
    v64 = [v.double().requires_grad_(True) for v in vols]
    outs = O.render(geom, *v64, seg_bounds=seg_bounds(cfg), output_coords=geo.output_coords,
                    camera_mids=geo.camera_mids, bev_mids=geo.bev_mids, d_far=cfg.d_bound[1],
                    z_step_det=cfg.z_bound_det[2], num_classes=cfg.num_classes, density_mode="sdf",
                    beta_param=torch.tensor(beta_v, dtype=F64), sdf_bias=cfg.sdf_bias, cat_seg=cfg.cat_seg,
                    compute_dtype=F64)
    ups = [u.double() for u in _upstream([o.shape for o in outs], seed, "cpu")]
    torch.autograd.backward(outs[:3], ups[:3])
    return {k: v.grad for k, v in zip(VOLS, v64) if k != "base"}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["thin-2x160x65", "dense-2x160x65-b3"])
def test_gather_overwrite_mode_above_the_gather_grid(dev, name):
    """The gather without VAMP_CAMBWD_ACCUMULATE stores every x-run (runs == nullptr) instead of adding the listed
    ones: HotPath never sends that, so a proxy clears the flag.  One stream, BEV call first; with the BEV outputs'
    upstream zero the BEV branch leaves zeros in the three shared buffers, and what the camera call overwrites them
    with is the whole gradient.  thin: 20 800 x-runs on a grid of 20 480, 320 workgroups store a second item of
    zeros; dense: 31 200 x-runs, 10 720 second items of which thousands hold visible gradient
    (test_items_carry_gradient)."""
    case = CASE_BY_NAME[name]
    cfg, rm, vols, beta_v = scene(case)
    ref = oracle_camera_only(case)
    hp = hot(cfg, dev)
    hp.impl.update(PATHS["merged"])
    hp.impl["overlap"] = False
    calls = hp.lib = _Overwrite(hp.lib)
    lv = [v.to(dev).requires_grad_(True) for v in vols]
    beta = torch.tensor(beta_v, device=dev, requires_grad=True)
    outs = hp.render(*lv, beta, render_mats=rm.to(dev))
    ups = _upstream([o.shape for o in outs], 4545, dev)
    ups = ups[:3] + [torch.zeros_like(u) for u in ups[3:]]
    torch.autograd.backward(outs, ups)
    bwd = [a for n, a in calls.log if n == "vamp_render_camera_backward_acc"]
    names = [n for n, _ in calls.log if "backward" in n]
    assert len(bwd) == 1 and names == ["vamp_render_bev_backward_ex", "vamp_render_camera_backward_acc"], names
    flags = bwd[0][-3]
    assert not flags & (_capi.VAMP_CAMBWD_ACCUMULATE | _capi.VAMP_CAMBWD_SPLAT | _capi.VAMP_CAMBWD_PART_RAY
                        | _capi.VAMP_CAMBWD_PART_GATHER | _capi.VAMP_CAMBWD_PART_HEAVY), flags
    p = _capi.VampCameraBackwardPlan()
    assert calls._lib.vamp_render_camera_backward_plan(C.byref(bwd[0][0]), 0, 1, flags, 0, bwd[0][-4], C.byref(p)) == 0
    assert (p.path, p.accumulate, p.gather_grid) == (_capi.VAMP_CAMPLAN_BWD_CELL, 0, GATHER_GRID), (p.path, p.accumulate, p.gather_grid)
    errs = {f"grad_{k}": rel_err(v.grad, ref[k]) for k, v in zip(VOLS, lv) if k != "base"}
    print(f"\noverwrite mode {name}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = [f"{k}: {e:.3e} > {bar_of(case, k, GRAD_BAR):.1e}" for k, e in errs.items() if not e <= bar_of(case, k, GRAD_BAR)]
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------- GPU: lift forward
@functools.lru_cache(maxsize=None)
def oracle_lift_forward(case):
    cfg, geo, lm, depth, feat, _ = lift_shapes.scene(case)
    return O.lift(depth.double(), feat.double(), geo.voxel_coords, None, None, None, None, cfg.final_dim, cfg.d_bound,
                  prepared=lm, compute_dtype=F64)


@pytest.mark.gpu
@pytest.mark.parametrize("case", lift_shapes.CASES, ids=lambda c: c.name)
def test_lift_forward_against_float64_oracle(dev, case):
    """hp.lift on the scenes of tests/test_lift_bwd_cell_shapes.py (which compares the gradients only): the forward
    without grad and the training forward (it also emits the backward's pairs) against the float64 oracle."""
    cfg, geo, lm, depth, feat, _ = lift_shapes.scene(case)
    ref = oracle_lift_forward(case)
    hp = hot(cfg, dev)
    lmd = lm.to(dev)
    with torch.no_grad():
        o0 = hp.lift(depth.to(dev), feat.to(dev), lmd)
    out = hp.lift(depth.to(dev).requires_grad_(True), feat.to(dev).requires_grad_(True), lmd)
    assert out.requires_grad and not o0.requires_grad
    errs = {"no-grad forward": rel_err(o0, ref), "forward": rel_err(out, ref)}
    print(f"\n{case.name}: " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = [f"{k}: {e:.3e} > {LIFT_BAR:.1e}" for k, e in errs.items() if not e <= LIFT_BAR]
    assert not bad, f"{case.name}:\n" + "\n".join(bad)
