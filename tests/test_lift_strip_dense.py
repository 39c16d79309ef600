"""The consume phase of the lift backward's strip gather (lift_bwd_cell.hip: lift_bwd_strip_kernel), which deals a
chunk's work by pair -- depth terms with lane = (pair, role), the feature gradient as 16 x 16 x 4 products of the fp32
matrix cores over blocks of four pairs -- against the float64 autograd of oracle/aten_oracle.py, at the shapes where
that dealing can go wrong:

  every case of test_lift_bwd_cell_shapes with each of the three chunk sizes (128 / 64 / 32 pairs: chunk ends inside
  cells and between the two cell rows of a strip); strips whose pair count is no multiple of four and four-pair blocks
  that hold pairs of both cell rows; a cell of more than 256 pairs at 32 pairs per chunk (big-cell: one pixel pair active
  over many chunks); role pixels outside the strip on both sides and a ragged last strip (fW16 / fW24 / fW22); C = 4, 8, 16
  and 32 (two channel chunks); D = 2 and no depth at all; bf16 inputs; the logits entry.

A CPU test asserts the properties the scenes are used for.  Scenes, oracle and error measure are those of
test_lift_bwd_cell_shapes; gradients are compared as max error over max magnitude.  The bound of a variant is twice the
error the commit before this phase was rewritten showed on it on an MI355X (PARENT_ERR, one run), and never above the
project's 1e-4.  The depth gradient is a sum of 64-bit integers and has the same bits on every run: asserted for two
backward calls over the same inputs, as it held for that commit.
The GPU tests take well under a second each on an MI355X; the float64 oracle of a case is computed once."""
import ctypes as C
import functools

import pytest
import torch

from oracle import aten_oracle as O
from vampire_amd import _capi as A
from vampire_amd.ops import lift_desc
from test_hip_parity import hot
from test_lift_bwd_cell_shapes import B, CASES, F64, PROJECT_BAR, Case, oracle, pairs, scene
from test_render_shape_sweep import library, rel_err

WPPS = (1, 4, 16)                                   # VAMP_LIFTBWD_WPP1 / WPP4 / WPP16
CAP = {1: 128, 4: 64, 16: 32}                       # pairs staged per chunk

# shared-cells with twice the voxel rows: its largest cell holds more than 256 pairs
BIG_CELL = Case("big-cell", x=(5.0, 7.0, 0.015625), y=(-0.4, 0.4, 0.1), z=(1.0, 2.0, 0.5), grid=(128, 8, 2))


def by_name(name):
    return next(c for c in CASES + [BIG_CELL] if c.name == name)


# (case, chunk flag, entry): "lift" probabilities in, "logits" the fused softmax backward, "nodepth" use_depth off,
# "bf16" 16-bit depth and features
VARIANTS = [(c.name, w, "lift") for c in CASES for w in WPPS]
VARIANTS += [("big-cell", 16, "lift"), ("big-cell", 1, "lift")]
VARIANTS += [("fW22", 1, "logits"), ("shared-cells", 16, "logits"), ("D2", 4, "logits"), ("C32", 16, "logits"),
             ("grid-16x16x5", 1, "nodepth"), ("fW24", 16, "nodepth"), ("C32", 4, "nodepth"),
             ("fW22", 1, "bf16"), ("C32", 16, "bf16"), ("shared-cells", 4, "bf16")]


def vid(v):
    return f"{v[0]}-wpp{v[1]}" + ("" if v[2] == "lift" else "-" + v[2])


# rel_err of the parent commit's strip gather against the float64 oracle, MI355X, one run
PARENT_ERR = {
    "grid-24x11x5-wpp1": {"grad depth": 8.732e-07, "grad feat": 5.321e-07},
    "grid-24x11x5-wpp4": {"grad depth": 8.732e-07, "grad feat": 5.321e-07},
    "grid-24x11x5-wpp16": {"grad depth": 8.732e-07, "grad feat": 5.321e-07},
    "grid-72x3x2-wpp1": {"grad depth": 3.275e-07, "grad feat": 4.916e-07},
    "grid-72x3x2-wpp4": {"grad depth": 3.275e-07, "grad feat": 4.916e-07},
    "grid-72x3x2-wpp16": {"grad depth": 3.275e-07, "grad feat": 4.916e-07},
    "grid-16x16x5-wpp1": {"grad depth": 6.543e-07, "grad feat": 6.069e-07},
    "grid-16x16x5-wpp4": {"grad depth": 6.543e-07, "grad feat": 6.069e-07},
    "grid-16x16x5-wpp16": {"grad depth": 6.543e-07, "grad feat": 6.069e-07},
    "cams-1-wpp1": {"grad depth": 8.628e-07, "grad feat": 3.545e-07},
    "cams-1-wpp4": {"grad depth": 8.628e-07, "grad feat": 3.545e-07},
    "cams-1-wpp16": {"grad depth": 8.628e-07, "grad feat": 3.545e-07},
    "cams-5-wpp1": {"grad depth": 6.979e-07, "grad feat": 9.172e-07},
    "cams-5-wpp4": {"grad depth": 6.979e-07, "grad feat": 9.172e-07},
    "cams-5-wpp16": {"grad depth": 6.979e-07, "grad feat": 9.172e-07},
    "cams-9-wpp1": {"grad depth": 9.129e-07, "grad feat": 6.997e-07},
    "cams-9-wpp4": {"grad depth": 9.129e-07, "grad feat": 6.997e-07},
    "cams-9-wpp16": {"grad depth": 9.129e-07, "grad feat": 6.997e-07},
    "C8-wpp1": {"grad depth": 7.988e-07, "grad feat": 7.300e-07},
    "C8-wpp4": {"grad depth": 7.988e-07, "grad feat": 7.300e-07},
    "C8-wpp16": {"grad depth": 7.988e-07, "grad feat": 7.300e-07},
    "C16-wpp1": {"grad depth": 7.145e-07, "grad feat": 7.152e-07},
    "C16-wpp4": {"grad depth": 7.145e-07, "grad feat": 7.152e-07},
    "C16-wpp16": {"grad depth": 7.145e-07, "grad feat": 7.152e-07},
    "C32-wpp1": {"grad depth": 8.686e-07, "grad feat": 1.074e-06},
    "C32-wpp4": {"grad depth": 8.686e-07, "grad feat": 1.074e-06},
    "C32-wpp16": {"grad depth": 8.686e-07, "grad feat": 1.074e-06},
    "shared-cells-wpp1": {"grad depth": 6.852e-07, "grad feat": 2.863e-07},
    "shared-cells-wpp4": {"grad depth": 6.852e-07, "grad feat": 3.342e-07},
    "shared-cells-wpp16": {"grad depth": 6.852e-07, "grad feat": 2.863e-07},
    "distinct-cells-wpp1": {"grad depth": 7.986e-06, "grad feat": 9.500e-06},
    "distinct-cells-wpp4": {"grad depth": 7.986e-06, "grad feat": 9.500e-06},
    "distinct-cells-wpp16": {"grad depth": 7.986e-06, "grad feat": 9.500e-06},
    "fW16-wpp1": {"grad depth": 2.080e-07, "grad feat": 1.434e-07},
    "fW16-wpp4": {"grad depth": 2.080e-07, "grad feat": 1.189e-07},
    "fW16-wpp16": {"grad depth": 2.080e-07, "grad feat": 1.187e-07},
    "fW24-wpp1": {"grad depth": 1.922e-06, "grad feat": 7.554e-07},
    "fW24-wpp4": {"grad depth": 1.922e-06, "grad feat": 7.554e-07},
    "fW24-wpp16": {"grad depth": 1.922e-06, "grad feat": 7.554e-07},
    "fW22-wpp1": {"grad depth": 8.978e-07, "grad feat": 8.462e-07},
    "fW22-wpp4": {"grad depth": 8.978e-07, "grad feat": 8.462e-07},
    "fW22-wpp16": {"grad depth": 8.978e-07, "grad feat": 7.719e-07},
    "D2-wpp1": {"grad depth": 8.456e-07, "grad feat": 1.580e-06},
    "D2-wpp4": {"grad depth": 8.456e-07, "grad feat": 1.580e-06},
    "D2-wpp16": {"grad depth": 8.456e-07, "grad feat": 1.580e-06},
    "big-cell-wpp16": {"grad depth": 2.683e-07, "grad feat": 6.701e-07},
    "big-cell-wpp1": {"grad depth": 2.683e-07, "grad feat": 7.162e-07},
    "fW22-wpp1-logits": {"grad depth": 9.372e-07, "grad feat": 7.917e-07},
    "shared-cells-wpp16-logits": {"grad depth": 4.937e-07, "grad feat": 2.809e-07},
    "D2-wpp4-logits": {"grad depth": 6.287e-07, "grad feat": 1.584e-06},
    "C32-wpp16-logits": {"grad depth": 7.542e-07, "grad feat": 1.023e-06},
    "grid-16x16x5-wpp1-nodepth": {"grad feat": 8.169e-07},
    "fW24-wpp16-nodepth": {"grad feat": 8.500e-07},
    "C32-wpp4-nodepth": {"grad feat": 7.364e-07},
    "fW22-wpp1-bf16": {"grad depth": 8.773e-07, "grad feat": 7.314e-07},
    "C32-wpp16-bf16": {"grad depth": 9.481e-07, "grad feat": 1.052e-06},
    "shared-cells-wpp4-bf16": {"grad depth": 7.020e-07, "grad feat": 3.573e-07},
}


def bound(v, what):
    return min(2.0 * PARENT_ERR[vid(v)][what], PROJECT_BAR)


# ---------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def oracle_logits(case):
    """The logits entry: the case's depth distribution as log-probabilities, softmax in float64."""
    cfg, geo, lm, depth, feat, gout = scene(case)
    x = depth.log().double().requires_grad_(True)
    f = feat.double().requires_grad_(True)
    out = O.lift(x.softmax(dim=2), f, geo.voxel_coords, None, None, None, None, cfg.final_dim, cfg.d_bound, prepared=lm,
                 compute_dtype=F64)
    out.backward(gout.double())
    return x.grad, f.grad


@functools.lru_cache(maxsize=None)
def oracle_bf16(case):
    """float64 autograd at the bf16-rounded inputs."""
    cfg, geo, lm, depth, feat, gout = scene(case)
    d = depth.bfloat16().double().requires_grad_(True)
    f = feat.bfloat16().double().requires_grad_(True)
    out = O.lift(d, f, geo.voxel_coords, None, None, None, None, cfg.final_dim, cfg.d_bound, prepared=lm,
                 compute_dtype=F64)
    out.backward(gout.double())
    return d.grad, f.grad


@functools.lru_cache(maxsize=None)
def nodepth(case):
    """use_depth off: the features alone are sampled (D = 1, every voxel in front of the camera counts).  Returns the
    upstream gradient -- none at the voxels whose samples are exact zeros -- and the float64 feature gradient."""
    cfg, geo, lm, depth, feat, gout = scene(case)
    pix = O.ego_to_pixel(geo.voxel_coords, None, None, None, None, lm)
    with torch.no_grad():
        valid, grid = O.lift_valid_and_grid(pix, cfg.final_dim, cfg.d_bound, use_depth=False)
        sm = torch.nn.functional.grid_sample(feat.unsqueeze(3).flatten(0, 1), grid.flatten(0, 1), align_corners=False)
        sm = sm.reshape(B, cfg.num_cams, cfg.mid_channels, *grid.shape[2:5])
        fragile = ((sm.abs() < 1e-7) & valid.bool().unsqueeze(2)).any(dim=1)
    g = gout.clone()
    g[fragile] = 0.0
    f = feat.double().requires_grad_(True)
    out = O.lift_from_frustum_feats(f.unsqueeze(3), pix, cfg.final_dim, cfg.d_bound, use_depth=False, compute_dtype=F64)
    out.backward(g.double())
    return g, f.grad


# ---------------------------------------------------------------------------------------------------- the kernel
def bf16_backward(case, wpp, dev):
    """Forward + backward through the C entry points with bf16 depth and features: the gradients come back as the
    kernel writes them, fp32 (the autograd wrapper would round them to the inputs' 16 bits)."""
    cfg, geo, lm, depth, feat, gout = scene(case)
    hp = hot(cfg, dev)
    lib = library()
    d = lift_desc(cfg, B, cfg.num_cams, cfg.mid_channels, A.VAMP_BF16)
    ws = torch.empty(lib.vamp_lift_workspace_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
    dep, ft = depth.to(dev).bfloat16().contiguous(), feat.to(dev).bfloat16().contiguous()
    lmd, go = lm.to(dev).float().contiguous(), gout.to(dev).contiguous()
    vox = torch.empty(B, cfg.mid_channels, cfg.vZ, cfg.vY, cfg.vX, device=dev)
    hits = torch.empty(B, cfg.vZ, cfg.vY, cfg.vX, (cfg.mid_channels + 15) // 16, dtype=torch.int64, device=dev)
    gd = torch.empty(dep.shape, dtype=torch.float32, device=dev)
    gf = torch.empty(ft.shape, dtype=torch.float32, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    geom = (ptr(lmd), ptr(hp.xs), ptr(hp.ys), ptr(hp.zs))
    rc = lib.vamp_lift_forward_ex(C.byref(d), *geom, ptr(dep), ptr(ft), ptr(vox), ptr(hits), ptr(ws), ws.numel(),
                                  A.VAMP_LIFTFWD_EMIT_PAIRS, None)
    assert rc == 0, lib.vamp_last_error().decode()
    flags = A.VAMP_LIFTBWD_CELLS_VALID | {1: A.VAMP_LIFTBWD_WPP1, 4: A.VAMP_LIFTBWD_WPP4, 16: A.VAMP_LIFTBWD_WPP16}[wpp]
    rc = lib.vamp_lift_backward_ex(C.byref(d), *geom, ptr(dep), ptr(ft), ptr(go), ptr(hits), ptr(gd), ptr(gf), ptr(ws),
                                   ws.numel(), flags, None)
    assert rc == 0, lib.vamp_last_error().decode()
    torch.cuda.synchronize()
    return gd, gf


def gradients(v, dev):
    """(gradient of the depth input or None, feature gradient) of the strip gather on a variant, and their references."""
    name, wpp, entry = v
    case = by_name(name)
    cfg, geo, lm, depth, feat, gout = scene(case)
    if entry == "bf16":
        return bf16_backward(case, wpp, dev) + oracle_bf16(case)
    hp = hot(cfg, dev)
    hp.impl["lift_bwd"] = "cell"
    hp.impl["lift_wpp"] = wpp
    f = feat.to(dev).requires_grad_(True)
    if entry == "nodepth":
        g, ref_gf = nodepth(case)
        hp.lift(None, f, lm.to(dev), use_depth=False).backward(g.to(dev))
        return None, f.grad, None, ref_gf
    x = (depth.log() if entry == "logits" else depth).to(dev).requires_grad_(True)
    (hp.lift_logits(x, f, lm.to(dev)) if entry == "logits" else hp.lift(x, f, lm.to(dev))).backward(gout.to(dev))
    return (x.grad, f.grad) + (oracle_logits(case) if entry == "logits" else oracle(case))


def errors(v, dev):
    gd, gf, ref_gd, ref_gf = gradients(v, dev)
    errs = {"grad feat": rel_err(gf, ref_gf)}
    if gd is not None:
        errs["grad depth"] = rel_err(gd, ref_gd)
    return errs


# ---------------------------------------------------------------------------------------------------- the scenes' properties
@functools.lru_cache(maxsize=None)
def strips(case):
    """Of every 16-pixel strip of the gather: (pairs of cell row iy in columns x0 .. x0 + np, pairs of cell row iy + 1
    there) -- the two ranges whose concatenation the strip stages in chunks -- and the largest cell of the scene."""
    cfg = case.cfg
    valid, cell = pairs(case)
    cw = cfg.fW + 1
    out, biggest = [], 0
    for b in range(B):
        for n in range(cfg.num_cams):
            cnt = torch.bincount(cell[b, n][valid[b, n]], minlength=(cfg.fH + 1) * cw).view(cfg.fH + 1, cw)
            biggest = max(biggest, int(cnt.max()))
            for x0 in range(0, cfg.fW, 16):
                cols = cnt[:, x0:x0 + min(16, cfg.fW - x0) + 1].sum(dim=1)
                out += [(int(cols[iy]), int(cols[iy + 1])) for iy in range(cfg.fH)]
    return out, biggest


def test_scenes_have_the_properties_the_dense_phase_needs():
    names = {v[0] for v in VARIANTS}
    assert names == {c.name for c in CASES} | {"big-cell"}
    assert {(n, w) for n, w, e in VARIANTS if e == "lift"} >= {(c.name, w) for c in CASES for w in WPPS}
    for c in CASES:
        st, _ = strips(c)
        # a last block of fewer than four pairs, and a block with pairs of both cell rows: the rows meet at n0, blocks
        # begin at multiples of four (every chunk size is one)
        assert any((n0 + n1) % 4 for n0, n1 in st), c.name
        assert any(n0 % 4 and n1 for n0, n1 in st), c.name
    # chunk ends inside the first cell row and the boundary of the two rows inside a later chunk: at every chunk size
    # in some strip of the dense scenes, at 32 pairs per chunk in each of them
    dense = {name: strips(by_name(name))[0] for name in ("fW16", "fW24", "fW22", "shared-cells")}
    crossing = lambda st, cap: any(n0 > cap and n0 % cap and n1 for n0, n1 in st)
    assert all(any(crossing(st, cap) for st in dense.values()) for cap in CAP.values())
    assert all(crossing(st, 32) for st in dense.values()), {n: crossing(st, 32) for n, st in dense.items()}
    # one cell of more than 256 pairs: at 32 pairs per chunk its two pixels alone are active for over eight chunks
    assert strips(BIG_CELL)[1] > 256 and ("big-cell", 16, "lift") in VARIANTS, strips(BIG_CELL)[1]
    # role pixels outside the strip on both sides (more than one strip per row) and a ragged last strip
    assert by_name("fW24").cfg.fW == 24 and by_name("fW22").cfg.fW == 22 and by_name("fW16").cfg.fW == 16
    assert by_name("C8").C == 8 and by_name("C16").C == 16 and by_name("C32").C == 32 and by_name("D2").cfg.D == 2
    assert set(PARENT_ERR) == {vid(v) for v in VARIANTS}
    assert all(set(PARENT_ERR[vid(v)]) == ({"grad feat"} if v[2] == "nodepth" else {"grad feat", "grad depth"})
               for v in VARIANTS)


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("v", VARIANTS, ids=vid)
def test_dense_consume_against_float64_oracle(dev, v):
    errs = errors(v, dev)
    for what, e in errs.items():
        print(f"{vid(v)} {what}: {e:.3e} (bound {bound(v, what):.3e})")
    bad = [f"{what}: {e:.3e} > {bound(v, what):.3e}" for what, e in errs.items() if not e <= bound(v, what)]
    assert not bad, f"{vid(v)}:\n" + "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("v", [("fW22", 1, "lift"), ("shared-cells", 16, "lift"), ("C32", 4, "lift")], ids=vid)
def test_depth_gradient_has_the_same_bits_every_run(dev, v):
    """Two forward + backward calls over the same inputs: the slots inside a cell follow the fill's atomics and differ,
    the fixed-point depth sums do not."""
    a, b = gradients(v, dev)[0], gradients(v, dev)[0]
    assert torch.equal(a, b), f"{vid(v)}: {int((a != b).sum())} of {a.numel()} depth gradients differ between two runs"
