"""The cell-list lift backward (lift_bwd_cell.hip: the fill, whose waves are 64 consecutive voxels of a sample's
flattened (z, y, x) index, and the strip gather) at the shapes where its code takes another path, against the float64
autograd of oracle/aten_oracle.py.

Every lift test at small size elsewhere has the 16 x 16 x 5 grid of CFG_TINY: one wave per row, no row end inside a
wave.  The cases here move one thing at a time from CFG_TINY: the grid (row and plane ends inside waves, a ragged last
wave, X above 64), the camera count (one, two, three batches of four; whole waves that no camera sees), the channel
count (every compiled fill body, two channel chunks in the strip), how many voxels share a cell (runs of 64 lanes that
continue in the next wave; no sharing at all), the feature-map width (a full strip, 16-byte tile I/O with a ragged strip,
scalar I/O; strips of more than 128 pairs, the staging chunk) and D = 2.  A CPU test asserts that each scene has the
property its case is named for.

Inputs follow tests/test_render_shape_sweep.py: exact zeros in one feature channel, no upstream gradient at the
voxels whose samples are exact zeros (they carry a 1e6 factor), B = 2 with a jittered rig.  Gradients are compared as
max error over max magnitude.  The bound of a case is twice the error that the cell backward of the commit before the
fill's waves were flattened showed on that case on an MI355X (PARENT_ERR, measured once); the factor covers the slot
order inside a cell, which follows the atomics and moves the last bits of the fp32 feature-gradient sums.  No bound is
above the project's 1e-4.
The GPU tests take about 3 s on an MI355X, the float64 oracle on the CPU included."""
import dataclasses
import functools

import pytest
import torch

from oracle import aten_oracle as O
from vampire_amd import synthetic
from vampire_amd.config import CFG_TINY
from vampire_amd.geometry import PathGeometry, lift_matrices
from test_hip_parity import hot
from test_render_shape_sweep import depth_bound, rel_err

F64 = torch.float64
PROJECT_BAR = 1e-4
B = 2


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    x: tuple = CFG_TINY.x_bound_seg
    y: tuple = CFG_TINY.y_bound_seg
    z: tuple = CFG_TINY.z_bound_seg
    grid: tuple = (16, 16, 5)            # (X, Y, Z) the bounds must give
    num_cams: int = 6
    C: int = 4
    final_dim: tuple = CFG_TINY.final_dim
    D: int = 21

    @property
    def cfg(self):
        cfg = dataclasses.replace(CFG_TINY, x_bound_seg=self.x, y_bound_seg=self.y, z_bound_seg=self.z,
                                  x_bound_det=self.x, y_bound_det=self.y, num_cams=self.num_cams,
                                  mid_channels=self.C, final_dim=self.final_dim,
                                  d_bound=CFG_TINY.d_bound if self.D == 21 else depth_bound(self.D - 1))
        assert (cfg.vX, cfg.vY, cfg.vZ) == self.grid and cfg.D == self.D, (cfg.vX, cfg.vY, cfg.vZ, cfg.D)
        return cfg


TALL = dict(z=(-2.0, 6.0, 0.8), grid=(16, 16, 10))                     # the planes above 4 m are seen by no camera
DENSE = dict(x=(-6.4, 6.4, 0.4), y=(-6.4, 6.4, 0.4), z=(-2.0, 2.0, 0.4), grid=(32, 32, 10))  # eight times the pairs per strip

CASES = [
    # ---- row ends inside waves
    Case("grid-24x11x5", x=(-6.0, 6.0, 0.5), y=(-2.75, 2.75, 0.5), grid=(24, 11, 5)),     # V = 1320: ragged last wave
    Case("grid-72x3x2", x=(-9.0, 9.0, 0.25), y=(-0.75, 0.75, 0.5), z=(-0.5, 1.5, 1.0), grid=(72, 3, 2)),
    Case("grid-16x16x5"),                                                                 # V = 1280 = 20 waves
    # ---- camera batches of four: one, two, three; whole waves without a camera
    Case("cams-1", num_cams=1, **TALL),
    Case("cams-5", num_cams=5, **TALL),
    Case("cams-9", num_cams=9, **TALL),
    # ---- the compiled fill bodies (C = 4: every case above), two channel chunks in the strip
    Case("C8", C=8),
    Case("C16", C=16),
    Case("C32", C=32),
    # ---- cell sharing
    Case("shared-cells", x=(5.0, 7.0, 0.015625), y=(-0.4, 0.4, 0.2), z=(1.0, 2.0, 0.5), grid=(128, 4, 2)),
    Case("distinct-cells", x=(-16.0, 16.0, 2.0), y=(-16.0, 16.0, 2.0), z=(-2.0, 4.0, 2.0), grid=(16, 16, 3),
         final_dim=(256, 704)),
    # ---- feature-map widths, strips of more than 128 pairs
    Case("fW16", final_dim=(32, 64), **DENSE),
    Case("fW24", final_dim=(32, 96), **DENSE),
    Case("fW22", **DENSE),
    # ---- D = 2
    Case("D2", D=2),
]

# rel_err of the parent commit's cell backward against the float64 oracle, MI355X, one run
PARENT_ERR = {
    "grid-24x11x5": {"grad depth": 8.732e-07, "grad feat": 5.321e-07},
    "grid-72x3x2": {"grad depth": 3.275e-07, "grad feat": 4.916e-07},
    "grid-16x16x5": {"grad depth": 6.543e-07, "grad feat": 6.069e-07},
    "cams-1": {"grad depth": 8.628e-07, "grad feat": 3.545e-07},
    "cams-5": {"grad depth": 6.979e-07, "grad feat": 9.172e-07},
    "cams-9": {"grad depth": 9.129e-07, "grad feat": 6.997e-07},
    "C8": {"grad depth": 7.988e-07, "grad feat": 7.300e-07},
    "C16": {"grad depth": 7.145e-07, "grad feat": 7.152e-07},
    "C32": {"grad depth": 8.686e-07, "grad feat": 1.074e-06},
    "shared-cells": {"grad depth": 6.852e-07, "grad feat": 3.102e-07},
    "distinct-cells": {"grad depth": 7.986e-06, "grad feat": 9.500e-06},
    "fW16": {"grad depth": 2.080e-07, "grad feat": 1.189e-07},
    "fW24": {"grad depth": 1.922e-06, "grad feat": 7.772e-07},
    "fW22": {"grad depth": 8.978e-07, "grad feat": 6.975e-07},
    "D2": {"grad depth": 8.456e-07, "grad feat": 1.580e-06},
}


def bound(case, what):
    return min(2.0 * PARENT_ERR[case.name][what], PROJECT_BAR)


@functools.lru_cache(maxsize=None)
def scene(case):
    """CPU tensors of a case, as test_render_shape_sweep.lift_scene makes them."""
    cfg = case.cfg
    s2e, intrin, ida = synthetic.camera_rig(cfg, B, jitter=1.0, seed=5)
    lm = lift_matrices(s2e, intrin, ida, synthetic.bda_matrix(B, rot_deg=5.0))
    gen = torch.Generator().manual_seed(700 + len(case.name) + case.C + case.D)
    logits = torch.randn(B, cfg.num_cams, cfg.D, cfg.fH, cfg.fW, generator=gen) * 2
    depth = logits.softmax(dim=2)
    feat = torch.randn(B, cfg.num_cams, cfg.mid_channels, cfg.fH, cfg.fW, generator=gen)
    feat[:, :, 1, ::3] = 0.0                     # exact zeros in a channel: the per-channel hit count
    geo = PathGeometry(cfg)
    with torch.no_grad():
        pix = O.ego_to_pixel(geo.voxel_coords, None, None, None, None, lm)
        valid, grid = O.lift_valid_and_grid(pix, cfg.final_dim, cfg.d_bound)
        ff = O.outer_depth_feat(depth, feat)
        sm = torch.nn.functional.grid_sample(ff.flatten(0, 1), grid.flatten(0, 1), align_corners=False)
        sm = sm.reshape(B, cfg.num_cams, cfg.mid_channels, *grid.shape[2:5])
        fragile = ((sm.abs() < 1e-7) & valid.bool().unsqueeze(2)).any(dim=1)
    gout = torch.randn(B, cfg.mid_channels, cfg.vZ, cfg.vY, cfg.vX, generator=gen)
    gout[fragile] = 0.0
    return cfg, geo, lm, depth, feat, gout


@functools.lru_cache(maxsize=None)
def oracle(case):
    """float64 autograd of the oracle lift: (grad depth, grad feat)."""
    cfg, geo, lm, depth, feat, gout = scene(case)
    d = depth.double().requires_grad_(True)
    f = feat.double().requires_grad_(True)
    out = O.lift(d, f, geo.voxel_coords, None, None, None, None, cfg.final_dim, cfg.d_bound, prepared=lm,
                 compute_dtype=F64)
    out.backward(gout.double())
    return d.grad, f.grad


def cell_backward_errors(case, dev):
    """Forward + backward of hp.lift with the cell-list backward: rel_err of both gradients against the oracle."""
    cfg, geo, lm, depth, feat, gout = scene(case)
    ref_gd, ref_gf = oracle(case)
    hp = hot(cfg, dev)
    hp.impl["lift_bwd"] = "cell"
    d = depth.to(dev).requires_grad_(True)
    f = feat.to(dev).requires_grad_(True)
    hp.lift(d, f, lm.to(dev)).backward(gout.to(dev))
    return {"grad depth": rel_err(d.grad, ref_gd), "grad feat": rel_err(f.grad, ref_gf)}


# ---------------------------------------------------------------------------------------------------- the scenes' properties
@functools.lru_cache(maxsize=None)
def pairs(case):
    """(valid [B, N, V] bool, cell [B, N, V]: row * (fW + 1) + column of the pair's cell) in flattened voxel order."""
    cfg, geo, lm = scene(case)[:3]
    pix = O.ego_to_pixel(geo.voxel_coords, None, None, None, None, lm)
    valid, ix0, iy0, _ = O.lift_tap_indices(pix, cfg.final_dim, cfg.d_bound, (cfg.D, cfg.fH, cfg.fW))
    cell = (iy0.long() + 1) * (cfg.fW + 1) + ix0.long() + 1
    return valid.flatten(2), cell.flatten(2)


def waves(t):
    """[B, N, V] -> [B, N, waves, 64], the ragged tail padded with -1 / False."""
    pad = (-t.shape[-1]) % 64
    fill = False if t.dtype == torch.bool else -1
    return torch.nn.functional.pad(t, (0, pad), value=fill).unflatten(-1, (-1, 64))


def longest_row_run(case):
    """The most x-consecutive voxels of one row that one camera puts into one cell."""
    valid, cell = pairs(case)
    X = case.grid[0]
    key = torch.where(valid, cell, torch.full_like(cell, -1)).unflatten(-1, (-1, X))
    best, run = 0, torch.zeros(key.shape[:-1], dtype=torch.long)
    for x in range(X):
        same = (key[..., x] >= 0) & (key[..., x] == key[..., x - 1]) if x else torch.zeros_like(run, dtype=torch.bool)
        run = torch.where(key[..., x] >= 0, torch.where(same, run + 1, torch.ones_like(run)), torch.zeros_like(run))
        best = max(best, int(run.max()))
    return best


def max_strip_pairs(case):
    """The most pairs that one 16-pixel strip of the gather reads: cell rows iy, iy + 1, columns x0 .. x0 + 16."""
    cfg = case.cfg
    valid, cell = pairs(case)
    cw = cfg.fW + 1
    best = 0
    for b in range(B):
        for n in range(cfg.num_cams):
            cnt = torch.bincount(cell[b, n][valid[b, n]], minlength=(cfg.fH + 1) * cw).view(cfg.fH + 1, cw)
            for x0 in range(0, cfg.fW, 16):
                cols = cnt[:, x0:x0 + 17].sum(dim=1)
                best = max(best, int((cols[:-1] + cols[1:]).max()))
    return best


def by_name(name):
    return next(c for c in CASES if c.name == name)


def test_scenes_have_the_properties_of_their_names():
    for c in CASES:
        X, Y, Z = c.grid
        V = X * Y * Z
        valid, cell = pairs(c)
        if c.name.startswith("grid-"):
            assert (64 % X != 0 and V % 64 != 0) == (c.name != "grid-16x16x5")
        if c.name.startswith("cams-"):
            seen = waves(valid).any(dim=3).any(dim=1)                    # [B, waves]
            assert (~seen).any() and seen.any(), f"{c.name}: no wave without a camera"
            assert (c.num_cams + 3) // 4 == {"cams-1": 1, "cams-5": 2, "cams-9": 3}[c.name]
            assert int(valid.any(dim=2).sum()) > 4 * ((c.num_cams - 1) // 4) * B, f"{c.name}: the last batch is empty"
    assert by_name("grid-72x3x2").grid[0] > 64
    assert longest_row_run(by_name("shared-cells")) > 64
    vd, cd = pairs(by_name("distinct-cells"))
    wv, wc = waves(vd), waves(torch.where(vd, cd, torch.full_like(cd, -1)))
    srt = wc.sort(dim=3).values
    assert not ((srt[..., 1:] == srt[..., :-1]) & (srt[..., 1:] >= 0)).any(), "distinct-cells: two lanes of a wave share a cell"
    assert int(wv.sum(dim=3).max()) >= 8, "distinct-cells: no wave with several pairs of one camera"
    for name in ("fW16", "fW24", "fW22"):
        c = by_name(name)
        assert c.cfg.fW == int(name[2:]) and max_strip_pairs(c) > 128, (name, max_strip_pairs(c))
    assert by_name("C32").C == 32 and by_name("D2").cfg.D == 2


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cell_backward_against_float64_oracle(dev, case):
    errs = cell_backward_errors(case, dev)
    for what, e in errs.items():
        print(f"{case.name} {what}: {e:.3e} (bound {bound(case, what):.3e})")
    bad = [f"{what}: {e:.3e} > {bound(case, what):.3e}" for what, e in errs.items() if not e <= bound(case, what)]
    assert not bad, f"{case.name}:\n" + "\n".join(bad)
