"""The render and lift kernels across the shape values that pick their compiled bodies and code paths -- the depth-bin
count S = D - 1, the class count K, the mid-channel count C, a ragged frustum and bf16 volumes -- against the oracle
evaluated in float64 (oracle/aten_oracle.py, compute_dtype): every output and every gradient, on each forced path.

One axis moves at a time from CFG_TINY (B = 2, six cameras).  The scene is the sdf workload with the low-x half of the
density volume turned into the "empty" regime (as tests/test_deep_tiles.py does), so rays that saturate within a few
samples share tiles with rays that run to the last depth index.

Bars are relative to the largest magnitude of the reference tensor and were set from the measured errors (at most ten
times the largest error seen over the sweep, never above the 1e-4 of the north star).  The CPU tests at the end hold the
render workspace's layout to the numbers of the commit before it had one definition, compare the library's camera plans
with Python mirrors, and fail if a compiled body is reached by no case.
The GPU tests of this file take about 4 s on an MI355X (the float64 oracle on the CPU included)."""
import ctypes as C
import dataclasses
import functools
import math

import pytest
import torch

from oracle import aten_oracle as O
from vampire_amd import _capi, synthetic
from vampire_amd.config import CFG_TINY
from vampire_amd.geometry import PathGeometry, lift_matrices, render_matrices
from test_hip_parity import NAMES, hot, _upstream
from test_deep_tiles import _term

F64 = torch.float64
VOLS = ("density_feature", "semantic_logits", "base", "rgb")

# ---------------------------------------------------------------------------------------------------- the sweep
DEPTHS = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 160]         # S = D - 1
CLASSES = [1, 5, 6, 9, 17, 18, 20, 21, 25, 28]                    # K
MIDS = [1, 4, 33, 64]                                             # C (and C = 0 beside cat_seg; without it, refused)
BF16_CLASSES = [5, 9, 18, 20, 28]                                 # one K per camera-forward body (NCH 8, 12, 21, 24, 32)
LIFT_DEPTHS = [2, 64, 65, 128, 129, 160]                          # D
PLAN_MAX = 128                                                    # kPlanMax (ray_plan.hpp)

# the forced paths: HotPath.impl switches (never "auto")
PATHS = {
    "merged": dict(cam_direct=True, ert=True, fwd_merged=True, cam_bwd="cell", save_rows=True),
    "two-launch": dict(cam_direct=True, ert=True, fwd_merged=False, cam_bwd="cell", save_rows=True),
    "direct-noert": dict(cam_direct=True, ert=False, fwd_merged=True, cam_bwd="cell", save_rows=True),
    "planned-ert": dict(cam_direct=False, ert=True, fwd_merged=True, cam_bwd="cell", save_rows=True),
    "planned-noert": dict(cam_direct=False, ert=False, fwd_merged=True, cam_bwd="cell", save_rows=True),
    "no-save-rows": dict(cam_direct=True, ert=True, fwd_merged=True, cam_bwd="cell", save_rows=False),
    "v1": dict(cam_direct=True, ert=True, fwd_merged=True, cam_bwd="v1", save_rows=True),
}

# bars: relative to max|reference| of the tensor (depth_preds: plus three fp32 roundings of sum w ~ 1 times d_far)
OUT_BAR = 1e-5
GRAD_BAR = 2e-5
BETA_BAR = 4e-6                      # grad_beta: relative to the sum of its terms' magnitudes (oracle_render); 4.8e-7 seen
BF16_GRAD_REL = 2.0 ** -8            # bf16 inputs get bf16 gradients: the fp32 result rounded once (8-bit significand)
LIFT_BAR = 2e-5                      # (the tap coordinates' fp32 rounding, ~1e-5 of a depth bin at D = 129: 4.6e-6 seen)
LIFT_GRAD_BAR = 3e-5


def depth_bound(S):
    """d_bound with D = S + 1 planes, a power-of-two step (every plane and mid exact), depths from 1 m to 9 - 13 m:
    across the 12.8 m grid whatever S."""
    step = 2.0 ** round(math.log2(10.0 / (S + 1)))
    return (1.0, 1.0 + (S + 1) * step, step)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    S: int = 20
    K: int = 5
    C: int = 4
    cat_seg: bool = False
    final_dim: tuple = (32, 88)
    bf16: bool = False

    @property
    def cfg(self):
        d_bound = CFG_TINY.d_bound if self.S == 20 else depth_bound(self.S)
        cfg = dataclasses.replace(CFG_TINY, density_mode="sdf", num_classes=self.K, mid_channels=self.C,
                                  cat_seg=self.cat_seg, final_dim=self.final_dim, d_bound=d_bound)
        assert cfg.D - 1 == self.S
        return cfg


CASES = ([Case(f"S{S}", S=S) for S in DEPTHS]
         + [Case(f"S160-K{K}", S=160, K=K) for K in (18, 28)]      # unplanned march / cell backward at CP 24, 32
         + [Case(f"K{K}-{'catseg' if cs else 'plain'}", K=K, cat_seg=cs) for K in CLASSES for cs in (False, True)]
         + [Case(f"C{C_}", C=C_) for C_ in MIDS] + [Case("C0-catseg", C=0, cat_seg=True)]
         + [Case("ragged-36x100", final_dim=(36, 100))]
         + [Case(f"bf16-K{K}", K=K, bf16=True) for K in BF16_CLASSES])


# ---------------------------------------------------------------------------------------------------- mirrors of the dispatch
def cam_direct_nch(K):
    """render_cam_direct_dev.hpp: cam_direct_nch(K + 3) -- the one-kernel and merged camera forwards' NCH."""
    n = K + 3
    return 8 if n <= 8 else (12 if n <= 12 else (21 if n == 21 else (24 if n <= 24 else 32)))


def channel_pack(K):
    """render_common.hpp: to_params -- CP, the packed channels of the march and the camera backwards."""
    need = 1 + K + 3
    return 12 if need <= 12 else (24 if need <= 24 else 32)


def ray_body(K):
    """render_bwd.hip: camera_backward_plan -- the per-ray backward's (CP / 4, KT) instance."""
    cp = channel_pack(K)
    return (cp // 4, 18 if (cp == 24 and K == 18) else 0)


def planned(S):
    return S <= PLAN_MAX


# ---------------------------------------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def scene(case):
    """CPU tensors: (cfg, render_mats [B,N,3,4,4], volumes (fp32, bf16-rounded for bf16 cases), beta).  A case may
    carry a batch size `B` (2 without) and a factor `empty` on the whole density volume instead of on its low-x half
    (tests/test_camera_cell_shapes.py: no ray terminates)."""
    cfg = case.cfg
    B = getattr(case, "B", 2)
    s2e, intrin, ida = synthetic.camera_rig(cfg, B, jitter=1.0, seed=5)
    bda = synthetic.bda_matrix(B, rot_deg=5.0)
    rm = render_matrices(s2e, intrin, ida, bda)
    vols = list(synthetic.render_inputs(cfg, B, seed=17))
    d = vols[0].clone()
    if getattr(case, "empty", None) is None:
        d[..., : d.shape[-1] // 2] *= 0.4     # the "empty" regime: s - bias ~ +0.6, sigma ~ 0.012 / m
    else:
        d *= case.empty
    vols[0] = d
    if case.bf16:
        vols = [v.bfloat16().float() for v in vols]
    return cfg, rm, vols, 0.1


@functools.lru_cache(maxsize=None)
def oracle_render(case, seed=4545):
    """float64 oracle: the eight outputs, the four volume gradients, grad_beta for the upstream of _upstream(), and
    the sum of the magnitudes of grad_beta's terms (one per sample and BEV cell: the scale of a one-element fp32 sum of
    mixed signs, whose value can cancel to a small fraction of its terms -- 0.043 of ~10 at S = 160, K = 18)."""
    cfg, rm, vols, beta_v = scene(case)
    terms, sdf = [], O.density_sdf

    def per_term_beta(s, beta_param, bias, beta_min=1e-4):
        b = beta_param.expand(s.shape)              # one beta per element: its gradient is that element's term
        b.retain_grad()
        terms.append(b)
        return sdf(s, b, bias, beta_min)
    geo = PathGeometry(cfg)
    geom = torch.nan_to_num(O.frustum_to_ego(geo.frustum, None, None, None, None, prepared=rm), -1e3)
    v64 = [v.double().requires_grad_(True) for v in vols]
    beta = torch.tensor(beta_v, dtype=F64, requires_grad=True)
    O.density_sdf = per_term_beta
    try:
        outs = O.render(geom, *v64, seg_bounds=(cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg),
                        output_coords=geo.output_coords, camera_mids=geo.camera_mids, bev_mids=geo.bev_mids,
                        d_far=cfg.d_bound[1], z_step_det=cfg.z_bound_det[2], num_classes=cfg.num_classes,
                        density_mode="sdf", beta_param=beta, sdf_bias=cfg.sdf_bias, cat_seg=cfg.cat_seg,
                        compute_dtype=F64)
    finally:
        O.density_sdf = sdf
    ups = [u.cpu().double() for u in _upstream([o.shape for o in outs], seed, "cpu")]
    torch.autograd.backward(outs, ups)
    assert len(terms) == 2                          # camera branch, BEV branch
    scale = sum(float(t.grad.abs().sum()) for t in terms)
    assert abs(sum(float(t.grad.sum()) for t in terms) - float(beta.grad)) <= 1e-9 * scale
    return [o.detach() for o in outs], [v.grad for v in v64], float(beta.grad), scale


class _Calls:
    """The library behind one HotPath, recording the render entry points it is called through (name, arguments)."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("vamp_render"):
            return fn

        def call(*a):
            self.log.append((name, a))
            return fn(*a)
        return call

    def flags(self, name, pos):
        return [a[pos] for n, a in self.log if n == name]


def rel_err(a, b):
    """max |a - b| / max |b| (b the float64 reference; 0 for empty tensors)."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def bf16_excess(a, b):
    """rel_err of a bf16 gradient beyond its own rounding: max (|a - b| - 2^-8 |b|)+ / max |b|."""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.numel() == 0:
        return 0.0
    return float(((a - b).abs() - BF16_GRAD_REL * b.abs()).clamp_min(0).max()) / max(float(b.abs().max()), 1e-30)


def run_path(case, path, dev, seed=4545):
    """One forced path on one case: (errors {what: (err, bar)}, calls).  Runs a no-grad forward and a training
    forward + backward on one HotPath."""
    cfg, rm, vols, beta_v = scene(case)
    ref_outs, ref_grads, ref_gbeta, gbeta_scale = oracle_render(case, seed)
    hp = hot(cfg, dev)
    hp.impl.update(PATHS[path])
    calls = hp.lib = _Calls(hp.lib)
    dt = torch.bfloat16 if case.bf16 else torch.float32
    dv = [v.to(dev, dt) for v in vols]
    rmd = rm.to(dev)
    errs = {}
    d_far = cfg.d_bound[1]

    def out_bar(nm, ref):
        if nm != "depth_preds":
            return OUT_BAR
        return OUT_BAR + 3 * 1.2e-7 * d_far / max(float(ref.abs().max()), 1e-30)

    with torch.no_grad():
        nog = hp.render(*dv, torch.tensor(beta_v, device=dev), render_mats=rmd)
    for nm, o, r in zip(NAMES, nog, ref_outs):
        errs[f"no-grad {nm}"] = (rel_err(o, r), out_bar(nm, r))
    lv = [v.clone().requires_grad_(True) for v in dv]
    beta = torch.tensor(beta_v, device=dev, requires_grad=True)
    outs = hp.render(*lv, beta, render_mats=rmd)
    for nm, o, r in zip(NAMES, outs, ref_outs):
        errs[f"train {nm}"] = (rel_err(o, r), out_bar(nm, r))
    torch.autograd.backward(outs, _upstream([o.shape for o in outs], seed, dev))
    for k, v, r in zip(VOLS, lv, ref_grads):
        assert v.grad.dtype == dt
        errs[f"grad_{k}"] = ((bf16_excess if case.bf16 else rel_err)(v.grad, r), GRAD_BAR)
    errs["grad_beta"] = (abs(float(beta.grad) - ref_gbeta) / gbeta_scale, BETA_BAR)
    return errs, calls


def check_path(case, path, calls, merged_ok=True):
    """The calls that ran are those of the path the case asked for (or, above kPlanMax, of its documented fallback;
    merged_ok False: the library does not offer the merged launch on the case's BEV geometry, the two launches run)."""
    S = case.S
    p = dict(PATHS[path], fwd_merged=PATHS[path]["fwd_merged"] and merged_ok)
    names = [n for n, _ in calls.log]
    fwd = calls.flags("vamp_render_camera_forward_ex", -2)
    mrg = calls.flags("vamp_render_forward_merged", -2)
    bwd = calls.flags("vamp_render_camera_backward_acc", -3)
    assert bwd, "no camera backward ran"
    if not planned(S):
        # no plan: the one-kernel forward, the merged launch, the planned march and save_rows are all off -- every path
        # runs the unplanned march and the unplanned cell backward
        assert not mrg and fwd and all(not (f & _capi.VAMP_CAMFWD_DIRECT) for f in fwd), (names, fwd)
        assert all(not (f & _capi.VAMP_CAMFWD_SAVE_SAMPLES) for f in fwd), fwd
        assert all(not (f & _capi.VAMP_CAMBWD_SAMPLES_VALID) for f in bwd), bwd
    elif p["cam_direct"] and not p["ert"]:
        # the one kernel without early termination: never merged (the merged launch terminates rays)
        assert not mrg and len(fwd) == 2 and all(f & _capi.VAMP_CAMFWD_DIRECT and f & _capi.VAMP_CAMFWD_NO_ERT
                                                 for f in fwd), (names, fwd)
        assert "vamp_render_camera_terminate" not in names, names
    elif p["cam_direct"] and p["fwd_merged"] and p["cam_bwd"] == "v1":
        # the v1 splat takes no cell lists: the training forward is the two launches, the no-grad one merged
        assert len(mrg) == 1 and len(fwd) == 1 and fwd[0] & _capi.VAMP_CAMFWD_DIRECT, (names, fwd)
        assert not (fwd[0] & _capi.VAMP_CAMFWD_SAVE_SAMPLES), fwd
    elif p["cam_direct"] and p["fwd_merged"]:
        assert len(mrg) == 2 and not fwd, names                   # no-grad call and training call: one launch each
        assert mrg[1] & _capi.VAMP_RENDERFWD_RANK, mrg
        assert bool(mrg[1] & _capi.VAMP_RENDERFWD_SAVE_SAMPLES) == p["save_rows"], mrg
    elif p["cam_direct"]:
        assert not mrg and len(fwd) == 2 and all(f & _capi.VAMP_CAMFWD_DIRECT for f in fwd), (names, fwd)
        assert "vamp_render_bev_forward_ex" in names
        # (the v1 splat reads no sample rows; it comes here only where the merged launch is not offered)
        assert bool(fwd[1] & _capi.VAMP_CAMFWD_SAVE_SAMPLES) == (p["save_rows"] and p["cam_bwd"] != "v1"), fwd
    else:
        marches = [f for f in fwd if not (f & _capi.VAMP_CAMFWD_PACK_ONLY)]
        assert not mrg and len(marches) == 2 and all(not (f & _capi.VAMP_CAMFWD_DIRECT) for f in marches), (names, fwd)
        assert all(bool(f & _capi.VAMP_CAMFWD_NO_ERT) == (not p["ert"]) for f in fwd), fwd
        assert ("vamp_render_camera_terminate" in names) == p["ert"], names
    if p["cam_bwd"] == "v1":
        assert all(f & _capi.VAMP_CAMBWD_SPLAT for f in bwd), bwd
    else:
        assert all(not (f & _capi.VAMP_CAMBWD_SPLAT) for f in bwd), bwd
        if planned(S) and p["save_rows"]:
            assert any(f & _capi.VAMP_CAMBWD_SAMPLES_VALID for f in bwd), bwd
        if not p["save_rows"]:
            assert all(not (f & _capi.VAMP_CAMBWD_SAMPLES_VALID) for f in bwd), bwd


# ---------------------------------------------------------------------------------------------------- GPU: render
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_render_sweep_against_float64_oracle(dev, case):
    """Each forced path: the eight outputs (no-grad and training forward), the four volume gradients and grad_beta
    against the float64 oracle; the C calls made are those of the path; the merged launch is offered exactly up to
    kPlanMax."""
    cfg = case.cfg
    hp = hot(cfg, dev)
    d = hp.render_desc(2, cfg.num_cams, _capi.VAMP_BF16 if case.bf16 else _capi.VAMP_F32)
    assert hp.lib.vamp_render_forward_merged_supported(C.byref(d), hp.ozs_host) == (1 if planned(case.S) else 0)
    bad = []
    for path in PATHS:
        errs, calls = run_path(case, path, dev)
        check_path(case, path, calls)
        bad += [f"{path} {what}: {e:.3e} > {b:.1e}" for what, (e, b) in errs.items() if not e <= b]
    assert not bad, f"{case.name}:\n" + "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.name.startswith("S") and c.S <= PLAN_MAX], ids=lambda c: c.name)
def test_depth_sweep_scene_exercises_the_scan(dev, case):
    """The termination table of the one-kernel forward holds indices in every residue mod 4 (for S >= 4; every index
    1 .. S below) -- the four-bins-ahead scan stops in each slot of its block -- and some rays keep all S samples."""
    cfg, rm, vols, beta_v = scene(case)
    hp = hot(cfg, dev)
    hp.impl.update(PATHS["merged"])
    with torch.no_grad():
        hp.render(*[v.to(dev) for v in vols], torch.tensor(beta_v, device=dev), render_mats=rm.to(dev))
    term = _term(hp, cfg, 2).cpu()
    S = case.S
    vals = set(term.flatten().tolist())
    assert vals <= set(range(0, S + 1)), sorted(vals)
    assert S in vals, "no ray keeps every sample"
    assert len({v % 4 for v in vals if v >= 1}) == min(4, S), sorted(vals)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["merged", "planned-ert"])
def test_backward_of_a_render_workspace_that_is_no_longer_fresh(dev, path):
    """A backward whose forward's leavings in the render workspace are gone promises the library none of them -- no
    PACKED / CELLS / TERM / SAMPLES_VALID on its camera calls -- and still gives every gradient within the sweep's bars:
    (a) ert_statistics between forward and backward (it overwrites the termination table), (b) the second backward of a
    retained graph (the first one scribbled over the cell lists)."""
    case = Case("tiny")
    cfg, rm, vols, beta_v = scene(case)
    _, ref_grads, ref_gbeta, gbeta_scale = oracle_render(case)
    promises = (_capi.VAMP_CAMBWD_PACKED_VALID | _capi.VAMP_CAMBWD_CELLS_VALID | _capi.VAMP_CAMBWD_TERM_VALID
                | _capi.VAMP_CAMBWD_SAMPLES_VALID)
    bad = []
    for route in ("ert-statistics", "second-backward"):
        hp = hot(cfg, dev)
        hp.impl.update(PATHS[path])
        calls = hp.lib = _Calls(hp.lib)
        lv = [v.to(dev).requires_grad_(True) for v in vols]
        beta = torch.tensor(beta_v, device=dev, requires_grad=True)
        rmd = rm.to(dev)
        outs = hp.render(*lv, beta, render_mats=rmd)
        ups = _upstream([o.shape for o in outs], 4545, dev)
        if route == "ert-statistics":
            hp.ert_statistics(lv[0].detach(), beta, rmd)
        else:
            torch.autograd.backward(outs, ups, retain_graph=True)
            fresh = calls.flags("vamp_render_camera_backward_acc", -3)
            assert fresh and all(f & promises for f in fresh), fresh        # (the first backward did find them)
            for t in lv + [beta]:
                t.grad = None
        n = len(calls.log)
        torch.autograd.backward(outs, ups)
        flags = [a[-3] for name, a in calls.log[n:] if name == "vamp_render_camera_backward_acc"]
        assert flags and all(not (f & promises) for f in flags), (route, flags)
        errs = {f"grad_{k}": (rel_err(v.grad, r), GRAD_BAR) for k, v, r in zip(VOLS, lv, ref_grads)}
        errs["grad_beta"] = (abs(float(beta.grad) - ref_gbeta) / gbeta_scale, BETA_BAR)
        bad += [f"{route} {what}: {e:.3e} > {b:.1e}" for what, (e, b) in errs.items() if not e <= b]
    assert not bad, f"{path}:\n" + "\n".join(bad)


@pytest.mark.gpu
def test_zero_mid_channels_need_cat_seg(dev):
    """C = 0 renders beside cat_seg (the sweep's C0-catseg case); without it voxel_output would have no channels and
    HotPath refuses the call before any device work."""
    cfg = Case("C0", C=0).cfg
    _, rm, vols, _ = scene(Case("C0-catseg", C=0, cat_seg=True))
    hp = hot(cfg, dev)
    with pytest.raises(ValueError, match="mid_channels = 0 needs cat_seg"):
        hp.render(*[v.to(dev) for v in vols], torch.tensor(0.1, device=dev), render_mats=rm.to(dev))


# ---------------------------------------------------------------------------------------------------- GPU: lift
@functools.lru_cache(maxsize=None)
def lift_scene(D):
    cfg = dataclasses.replace(CFG_TINY, d_bound=depth_bound(D - 1))
    assert cfg.D == D
    s2e, intrin, ida = synthetic.camera_rig(cfg, 2, jitter=1.0, seed=5)
    lm = lift_matrices(s2e, intrin, ida, synthetic.bda_matrix(2, rot_deg=5.0))
    gen = torch.Generator().manual_seed(300 + D)
    logits = torch.randn(2, cfg.num_cams, D, cfg.fH, cfg.fW, generator=gen) * 2
    feat = torch.randn(2, cfg.num_cams, cfg.mid_channels, cfg.fH, cfg.fW, generator=gen)
    feat[:, :, 1, ::3] = 0.0                     # exact zeros in a channel: the per-channel hit count (bv2:509-512)
    geo = PathGeometry(cfg)
    # voxels whose only samples are exact zeros carry a 1e6 factor (bv2:512): no upstream gradient there
    with torch.no_grad():
        pix = O.ego_to_pixel(geo.voxel_coords, None, None, None, None, lm)
        valid, grid = O.lift_valid_and_grid(pix, cfg.final_dim, cfg.d_bound)
        ff = O.outer_depth_feat(logits.softmax(dim=2), feat)
        B, N = 2, cfg.num_cams
        sm = torch.nn.functional.grid_sample(ff.flatten(0, 1), grid.flatten(0, 1), align_corners=False)
        sm = sm.reshape(B, N, cfg.mid_channels, *grid.shape[2:5])
        fragile = ((sm.abs() < 1e-7) & valid.bool().unsqueeze(2)).any(dim=1)
    gout = torch.randn(B, cfg.mid_channels, cfg.vZ, cfg.vY, cfg.vX, generator=gen)
    gout[fragile] = 0.0
    return cfg, geo, lm, logits, feat, gout


@functools.lru_cache(maxsize=None)
def oracle_lift(D, entry):
    """float64 oracle lift: forward, gradient of its depth input (probabilities, or the logits: softmax in float64)
    and of the features."""
    cfg, geo, lm, logits, feat, gout = lift_scene(D)
    if entry == "lift":
        x = logits.softmax(dim=2).double().requires_grad_(True)
        depth = x
    else:
        x = logits.to(torch.bfloat16 if entry == "logits-bf16" else torch.float32).double().requires_grad_(True)
        depth = x.softmax(dim=2)
    f = feat.double().requires_grad_(True)
    out = O.lift(depth, f, geo.voxel_coords, None, None, None, None, cfg.final_dim, cfg.d_bound, prepared=lm,
                 compute_dtype=F64)
    out.backward(gout.double())
    return out.detach(), x.grad, f.grad


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["lift", "logits-f32", "logits-bf16"])
@pytest.mark.parametrize("D", LIFT_DEPTHS)
def test_lift_depth_sweep_against_float64_oracle(dev, D, entry):
    """The lift (depth probabilities in) and the lift fed with depth logits (f32 / bf16; D > 128 runs the operand
    kernel's non-register path) against the float64 oracle: forward, depth or logits gradient and feature gradient,
    with the cell-list backward and with the v1 splat."""
    cfg, geo, lm, logits, feat, gout = lift_scene(D)
    ldtype = torch.bfloat16 if entry == "logits-bf16" else torch.float32
    use_logits = entry != "lift"
    x_in = logits.to(ldtype) if use_logits else logits.softmax(dim=2)
    ref_out, ref_gx, ref_gf = oracle_lift(D, entry)
    bad = []
    for impl in ("cell", "v1"):
        hp = hot(cfg, dev)
        hp.impl["lift_bwd"] = impl
        lmd = lm.to(dev)
        with torch.no_grad():
            o0 = (hp.lift_logits if use_logits else hp.lift)(x_in.to(dev), feat.to(dev), lmd)
        x = x_in.to(dev).requires_grad_(True)
        f = feat.to(dev).requires_grad_(True)
        out = (hp.lift_logits if use_logits else hp.lift)(x, f, lmd)
        out.backward(gout.to(dev))
        errs = {"no-grad forward": (rel_err(o0, ref_out), LIFT_BAR), "forward": (rel_err(out, ref_out), LIFT_BAR),
                "grad feat": (rel_err(f.grad, ref_gf), LIFT_GRAD_BAR)}
        assert x.grad.dtype == ldtype
        errs["grad " + ("depth" if entry == "lift" else entry)] = \
            ((bf16_excess if ldtype == torch.bfloat16 else rel_err)(x.grad, ref_gx), LIFT_GRAD_BAR)
        bad += [f"{impl} {w}: {e:.3e} > {b:.1e}" for w, (e, b) in errs.items() if not e <= b]
    assert not bad, f"D={D} {entry}:\n" + "\n".join(bad)


# ---------------------------------------------------------------------------------------------------- CPU: layout, plans
def case_desc(case, bf16=None):
    """The render descriptor of a sweep case as the GPU tests build it (B = 2); host only."""
    from vampire_amd.ops import render_desc
    cfg = case.cfg
    return render_desc(cfg, 2, cfg.num_cams, _capi.VAMP_BF16 if (case.bf16 if bf16 is None else bf16) else _capi.VAMP_F32)


@functools.lru_cache(maxsize=None)
def library():
    from vampire_amd.build import build_library
    build_library(verbose=False)
    return _capi.load()


def ws_layout(d):
    """vamp_render_workspace_layout: ({region: (offset, bytes)} in layout order, base_bytes, bytes_with_rows)."""
    out = _capi.VampRenderWorkspaceLayout()
    assert library().vamp_render_workspace_layout(C.byref(d), C.byref(out)) == 0
    return ({n: (out.offset[i], out.bytes[i]) for i, n in enumerate(_capi.RENDERWS_REGIONS)}, out.base_bytes,
            out.bytes_with_rows)


# (vamp_render_workspace_bytes, vamp_render_term_offset, vamp_render_samples_bytes) of the commit before the layout
# became cam_workspace() (2326e0f, built and asked on the CPU; f32 and bf16 descriptors give the same numbers): the
# sweep's cases at B = 2 and the presets A, B, D at batch 1 and 8.  The layout was moved, not changed.
PARENT_LAYOUT = {
    "S1": (414208, 405760, 110592),
    "S2": (526592, 518144, 221184),
    "S3": (638976, 630528, 331776),
    "S4": (751360, 742912, 442368),
    "S5": (863744, 855296, 552960),
    "S63": (7383808, 7375360, 6967296),
    "S64": (7496192, 7487744, 7077888),
    "S65": (7608832, 7600384, 7188480),
    "S127": (14578432, 14569984, 14045184),
    "S128": (14690816, 14682368, 14155776),
    "S129": (14803456, 14795008, 14266368),
    "S160": (18288128, 18279680, 17694720),
    "S160-K18": (22568192, 22559744, 35389440),
    "S160-K28": (25421568, 25413120, 47185920),
    "K1-plain": (2550016, 2541568, 2211840),
    "K1-catseg": (2550016, 2541568, 2211840),
    "K5-plain": (2550016, 2541568, 2211840),
    "K5-catseg": (2550016, 2541568, 2211840),
    "K6-plain": (2550016, 2541568, 2211840),
    "K6-catseg": (2550016, 2541568, 2211840),
    "K9-plain": (3281920, 3273472, 4423680),
    "K9-catseg": (3281920, 3273472, 4423680),
    "K17-plain": (3281920, 3273472, 4423680),
    "K17-catseg": (3281920, 3273472, 4423680),
    "K18-plain": (3281920, 3273472, 4423680),
    "K18-catseg": (3281920, 3273472, 4423680),
    "K20-plain": (3281920, 3273472, 4423680),
    "K20-catseg": (3281920, 3273472, 4423680),
    "K21-plain": (3769856, 3761408, 5898240),
    "K21-catseg": (3769856, 3761408, 5898240),
    "K25-plain": (3769856, 3761408, 5898240),
    "K25-catseg": (3769856, 3761408, 5898240),
    "K28-plain": (3769856, 3761408, 5898240),
    "K28-catseg": (3769856, 3761408, 5898240),
    "C1": (2550016, 2541568, 2211840),
    "C4": (2550016, 2541568, 2211840),
    "C33": (2550016, 2541568, 2211840),
    "C64": (2550016, 2541568, 2211840),
    "C0-catseg": (2550016, 2541568, 2211840),
    "ragged-36x100": (3719424, 3708416, 5898240),
    "bf16-K5": (2550016, 2541568, 2211840),
    "bf16-K9": (3281920, 3273472, 4423680),
    "bf16-K18": (3281920, 3273472, 4423680),
    "bf16-K20": (3281920, 3273472, 4423680),
    "bf16-K28": (3769856, 3761408, 5898240),
    "A-b1": (522648320, 522377984, 551485440),
    "A-b8": (4181004800, 4178842112, 4411883520),
    "B-b1": (446974464, 446704128, 551485440),
    "B-b8": (3575611648, 3573448960, 4411883520),
    "D-b1": (2074865664, 2073784320, 2205941760),
    "D-b8": (16598680320, 16590029568, 17647534080),
}


def layout_descs():
    from vampire_amd.config import PRESETS
    from vampire_amd.ops import render_desc
    for bf16 in (False, True):
        dt = _capi.VAMP_BF16 if bf16 else _capi.VAMP_F32
        for c in CASES:
            yield c.name, case_desc(c, bf16)
        for preset in "ABD":
            for B in (1, 8):
                yield f"{preset}-b{B}", render_desc(PRESETS[preset], B, PRESETS[preset].num_cams, dt)


def test_workspace_layout_is_the_parents():
    """The three byte queries answer what the parent commit answered, and the regions behind them are in order,
    256-byte aligned and disjoint (the v1 gradient copy overlays Gcl .. beta_part by design) and add up to the totals."""
    lib = library()
    n = 0
    for name, d in layout_descs():
        got = (lib.vamp_render_workspace_bytes(C.byref(d)), lib.vamp_render_term_offset(C.byref(d)),
               lib.vamp_render_samples_bytes(C.byref(d)))
        assert got == PARENT_LAYOUT[name], (name, got, PARENT_LAYOUT[name])
        regions, base_bytes, with_rows = ws_layout(d)
        assert list(regions) == list(_capi.RENDERWS_REGIONS)
        assert all(off % 256 == 0 and nb % 256 == 0 and nb > 0 for off, nb in regions.values()), (name, regions)
        at = 0
        for r in _capi.RENDERWS_REGIONS:                      # back to back, but for the overlay and the slack behind it
            off, nb = regions[r]
            if r == "grad":
                assert off == regions["packed"][1] and nb == regions["packed"][1], (name, regions)
                continue
            if r == "term":
                at = max(at, sum(regions["grad"]))
            assert off == at, (name, r, off, at)
            at += nb
        assert sum(regions["term"]) == base_bytes == got[0] and regions["term"][0] == got[1], (name, regions)
        assert regions["rows"] == (base_bytes, got[2]) and with_rows == base_bytes + got[2], (name, regions)
        n += 1
    assert n == 2 * len(PARENT_LAYOUT)
    assert lib.vamp_render_workspace_layout(None, C.byref(_capi.VampRenderWorkspaceLayout())) == -1
    assert lib.vamp_render_workspace_layout(C.byref(case_desc(Case("tiny"))), None) == -1


SCAN_TILE, RUN_VOX, GATHER_GRID, SPLAT_NW = 2048, 32, 20480, 2     # common.hpp, render_common.hpp, cam_lists.hpp
FWD_FIELDS = [n for n, _ in _capi.VampCameraForwardPlan._fields_]
BWD_FIELDS = [n for n, _ in _capi.VampCameraBackwardPlan._fields_]
ENOSPC, EINVAL = -2, -1
ERR_CELLS = "requirement failed: CELLS_VALID with early termination needs TERM_VALID"
ERR_COUNT = "requirement failed: sample / voxel / cell count exceeds 2^31"
ERR_LDS = "too many depth samples for the LDS staging"
ERR_RUNS = "requirement failed: too many x-runs"
ERR_SPLAT = "requirement failed: accumulate / wait_event need the cell-list path"


def shape_numbers(d):
    """What both plans take from the descriptor alone."""
    tiles = d.B * d.N * ((d.fH + 7) // 8) * ((d.fW + 7) // 8)
    ncell = d.B * (d.Z + 1) * (d.Y + 1) * (d.X + 1) + 2
    ncell = (ncell + SCAN_TILE - 1) // SCAN_TILE * SCAN_TILE
    runs = ((d.X + RUN_VOX - 1) // RUN_VOX) * d.Y * d.Z * d.B
    regions, base_bytes, with_rows = ws_layout(d)
    return dict(S=d.D - 1, K=d.K, cp=channel_pack(d.K), ray_grid=(tiles + 7) // 8 * 8, ncell=ncell, runs=runs,
                rays=d.B * d.N * d.fH * d.fW, voxels=d.B * d.Z * d.Y * d.X, sdf=d.density_mode == _capi.VAMP_DENSITY_SDF_LAPLACE,
                packed=regions["packed"][1], base=base_bytes, rows=with_rows)


def fwd_plan(n, has_geom, flags, ws_bytes):
    """render_fwd.hip: camera_forward_plan -- the fields of VampCameraForwardPlan, or (code, message tail)."""
    A = _capi
    p = dict.fromkeys(FWD_FIELDS, 0)
    plan = not has_geom and planned(n["S"])
    p["save_rows"] = int(bool(flags & A.VAMP_CAMFWD_SAVE_SAMPLES) and plan)
    p["ert"] = int(plan and not flags & A.VAMP_CAMFWD_NO_ERT)
    p["grid"] = n["ray_grid"]
    if flags & A.VAMP_CAMFWD_DIRECT and plan:
        p.update(path=A.VAMP_CAMPLAN_FWD_DIRECT, bytes_needed=n["rows"] if p["save_rows"] else 0,
                 term=A.VAMP_CAMPLAN_TERM_WRITE if ws_bytes >= n["base"] else A.VAMP_CAMPLAN_TERM_NONE,
                 body=cam_direct_nch(n["K"]))
    else:
        p.update(path=A.VAMP_CAMPLAN_FWD_PLANNED if plan else A.VAMP_CAMPLAN_FWD_MARCH,
                 bytes_needed=n["rows"] if p["save_rows"] else (n["base"] if p["ert"] else n["packed"]),
                 term=A.VAMP_CAMPLAN_TERM_NONE if not p["ert"] else
                 (A.VAMP_CAMPLAN_TERM_CHECK if flags & A.VAMP_CAMFWD_TERM_VALID else A.VAMP_CAMPLAN_TERM_BUILD),
                 pack=int(not flags & A.VAMP_CAMFWD_PACKED_VALID), pack_only=int(bool(flags & A.VAMP_CAMFWD_PACK_ONLY)),
                 body=n["cp"] // 4)
        if p["pack_only"]:
            p["body"] = p["grid"] = 0
    if ws_bytes < p["bytes_needed"]:
        return ENOSPC, f": workspace {ws_bytes} < {p['bytes_needed']} bytes"
    return p


def bwd_plan(n, has_geom, has_mats, flags, has_wait, ws_bytes):
    """render_bwd.hip: camera_backward_plan -- the fields of VampCameraBackwardPlan, or (code, message tail): the
    refusals in the order the library makes them."""
    A = _capi
    p = dict.fromkeys(BWD_FIELDS, 0)
    p["bytes_needed"] = n["base"]
    if ws_bytes < n["base"]:
        return ENOSPC, f": workspace {ws_bytes} < {n['base']} bytes"
    p["accumulate"] = int(bool(flags & A.VAMP_CAMBWD_ACCUMULATE))
    part_ray = not flags & (A.VAMP_CAMBWD_PART_GATHER | A.VAMP_CAMBWD_PART_HEAVY) or bool(flags & A.VAMP_CAMBWD_PART_RAY)
    if has_geom or not has_mats or flags & A.VAMP_CAMBWD_SPLAT:
        if p["accumulate"] or has_wait:
            return EINVAL, ERR_SPLAT
        p.update(path=A.VAMP_CAMPLAN_BWD_SPLAT, pack=int(not flags & A.VAMP_CAMBWD_PACKED_VALID and part_ray),
                 splat_grid=(n["rays"] + 255) // 256, unpack_grid=(n["voxels"] + 255) // 256)
        return p
    parts = ((1 if flags & A.VAMP_CAMBWD_PART_RAY else 0) | (2 if flags & A.VAMP_CAMBWD_PART_GATHER else 0)
             | (4 if flags & A.VAMP_CAMBWD_PART_HEAVY else 0)) or 7
    p.update(path=A.VAMP_CAMPLAN_BWD_CELL, parts=parts)
    if flags & A.VAMP_CAMBWD_SAMPLES_VALID:
        p["bytes_needed"] = n["rows"]
        if ws_bytes < n["rows"]:
            return ENOSPC, f": workspace {ws_bytes} has no room for the sample rows"
    p["beta_tail"] = int(n["sdf"] and bool(parts & 2))
    if part_ray:
        p["samples"] = int(bool(flags & A.VAMP_CAMBWD_SAMPLES_VALID))
        p["prepare"] = int(not flags & A.VAMP_CAMBWD_CELLS_VALID)
        if not flags & A.VAMP_CAMBWD_NO_ERT:
            p["term"] = A.VAMP_CAMPLAN_TERM_CHECK if flags & A.VAMP_CAMBWD_TERM_VALID else A.VAMP_CAMPLAN_TERM_BUILD
            if p["term"] == A.VAMP_CAMPLAN_TERM_BUILD and not p["prepare"]:
                return EINVAL, ERR_CELLS
        if p["prepare"] and not (0 < n["rays"] * n["S"] < 2 ** 31 - 1 and n["voxels"] < 2 ** 31 - 1 and n["ncell"] < 2 ** 31 - 1):
            return EINVAL, ERR_COUNT
        p["ray_cp4"], p["ray_kt"] = ray_body(n["K"])
        p["ray_lds"] = 3 * ((n["S"] + 3) // 4) * 256 * 4
        if p["ray_lds"] > 150 * 1024:
            return EINVAL, ERR_LDS
        p["raise_lds"] = int(p["ray_lds"] > 64 * 1024)
        p["ray_grid"] = n["ray_grid"]
        p["list_grid"] = n["ncell"] // SCAN_TILE + (n["runs"] + 255) // 256
    elif p["beta_tail"]:
        p["ray_grid"] = n["ray_grid"]
    if parts & 6:
        if n["runs"] >= 2 ** 31 - 1:
            return EINVAL, ERR_RUNS
        if parts & 4:
            p.update(heavy_grid=min(n["ncell"], 4096), heavy_waves={12: 2, 24: SPLAT_NW, 32: 4}[n["cp"]])
        if parts & 2:
            p["gather_grid"] = min(n["runs"], GATHER_GRID)
    return p


def ask(fn, struct, *args):
    """A plan entry point's answer in the mirrors' form: the struct, or (code, whole message)."""
    out = struct()
    rc = fn(*args, C.byref(out))
    return out if rc == 0 else (rc, library().vamp_last_error().decode())


def same_plan(got, want, struct, what):
    """The library's answer `got` is the mirror's `want`: every field, or the refusal's code and message tail."""
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and got[0] == want[0] and got[1].endswith(want[1]), (what, got, want)
        return
    assert not isinstance(got, tuple), (what, got, want)
    if bytes(got) != bytes(struct(**{k: v for k, v in want.items() if k != "reserved"})):
        diff = {k: (getattr(got, k), v) for k, v in want.items() if k != "reserved" and getattr(got, k) != v}
        assert not diff and list(got.reserved) == [0] * 6, (what, diff)


def subsets(bits):
    return [sum(b for i, b in enumerate(bits) if m >> i & 1) for m in range(1 << len(bits))]


def test_camera_plans_are_the_mirrors():
    """vamp_render_camera_forward_plan and vamp_render_camera_backward_plan -- the functions the two entry points ask
    before their first launch -- answer what the mirrors predict, field by field and refusal by refusal: every case x
    geom / mats x every combination of the flags x a workspace one byte below and exactly at each size that matters."""
    lib, A = library(), _capi
    fwd_flags = subsets([A.VAMP_CAMFWD_NO_ERT, A.VAMP_CAMFWD_TERM_VALID, A.VAMP_CAMFWD_PACK_ONLY,
                         A.VAMP_CAMFWD_PACKED_VALID, A.VAMP_CAMFWD_DIRECT, A.VAMP_CAMFWD_SAVE_SAMPLES])
    bwd_flags = subsets([A.VAMP_CAMBWD_ACCUMULATE, A.VAMP_CAMBWD_PACKED_VALID, A.VAMP_CAMBWD_CELLS_VALID,
                         A.VAMP_CAMBWD_SPLAT, A.VAMP_CAMBWD_SAMPLES_VALID, A.VAMP_CAMBWD_TERM_VALID,
                         A.VAMP_CAMBWD_NO_ERT, A.VAMP_CAMBWD_PART_RAY, A.VAMP_CAMBWD_PART_GATHER,
                         A.VAMP_CAMBWD_PART_HEAVY])
    assert len(fwd_flags) == 64 and len(bwd_flags) == 1024
    seen = {k: set() for k in ("fwd path", "fwd term", "fwd body", "bwd path", "bwd term", "raise_lds", "refusal")}
    for case in CASES:
        d = case_desc(case)
        n = shape_numbers(d)
        ref = C.byref(d)
        for has_geom in (0, 1):
            for ws in (0, n["packed"] - 1, n["packed"], n["base"] - 1, n["base"], n["rows"] - 1, n["rows"]):
                for f in fwd_flags:
                    got = ask(lib.vamp_render_camera_forward_plan, A.VampCameraForwardPlan, ref, has_geom, f, ws)
                    want = fwd_plan(n, has_geom, f, ws)
                    same_plan(got, want, A.VampCameraForwardPlan, (case.name, has_geom, f, ws))
                    if isinstance(want, dict):
                        seen["fwd path"].add(want["path"]), seen["fwd term"].add(want["term"])
                        seen["fwd body"].add((want["path"], want["body"]))
        for has_geom, has_mats in ((0, 1), (1, 0), (1, 1)):
            for ws in (n["base"] - 1, n["base"], n["rows"] - 1, n["rows"]):
                for f in bwd_flags:
                    got = ask(lib.vamp_render_camera_backward_plan, A.VampCameraBackwardPlan, ref, has_geom, has_mats, f, 0, ws)
                    want = bwd_plan(n, has_geom, has_mats, f, 0, ws)
                    same_plan(got, want, A.VampCameraBackwardPlan, (case.name, has_geom, has_mats, f, ws))
                    if isinstance(want, dict):
                        seen["bwd path"].add(want["path"]), seen["bwd term"].add(want["term"])
                        seen["raise_lds"].add(want["raise_lds"])
                    else:
                        seen["refusal"].add(want[1] if want[0] == EINVAL else "ENOSPC")
        # wait_event: refused on the splat with or without ACCUMULATE, nothing to the cell path's plan
        for f in (0, A.VAMP_CAMBWD_ACCUMULATE, A.VAMP_CAMBWD_SPLAT, A.VAMP_CAMBWD_SPLAT | A.VAMP_CAMBWD_ACCUMULATE):
            for has_geom in (0, 1):
                got = ask(lib.vamp_render_camera_backward_plan, A.VampCameraBackwardPlan, ref, has_geom, 1, f, 1, n["rows"])
                same_plan(got, bwd_plan(n, has_geom, 1, f, 1, n["rows"]), A.VampCameraBackwardPlan, (case.name, has_geom, f))
    assert seen["fwd path"] == {0, 1, 2} and seen["fwd term"] == {0, 1, 2, 3} and seen["bwd path"] == {0, 1}
    assert seen["bwd term"] == {0, 1, 2} and seen["raise_lds"] == {0, 1}
    assert seen["refusal"] == {"ENOSPC", ERR_CELLS, ERR_SPLAT}, seen["refusal"]


def test_camera_plan_refusals():
    """Each refusal of the two plans by code and message -- on descriptors no sweep case reaches: more than 2^31
    samples, more than 200 depth samples, more x-runs than a grid index -- and a NULL descriptor or plan."""
    lib, A = library(), _capi
    huge = 1 << 62

    def bwd(d, flags=0, geom=0, wait=0, ws=huge):
        return ask(lib.vamp_render_camera_backward_plan, A.VampCameraBackwardPlan, C.byref(d), geom, 1, flags, wait, ws)

    def refused(got, code, tail):
        assert isinstance(got, tuple) and got[0] == code and got[1].endswith(tail), (got, code, tail)

    tiny = case_desc(Case("tiny"))
    n = shape_numbers(tiny)
    refused(bwd(tiny, ws=n["base"] - 1), ENOSPC, f"vamp_render_camera_backward_plan: workspace {n['base'] - 1} < {n['base']} bytes")
    refused(bwd(tiny, A.VAMP_CAMBWD_SAMPLES_VALID, ws=n["rows"] - 1), ENOSPC,
            f"workspace {n['rows'] - 1} has no room for the sample rows")
    refused(bwd(tiny, A.VAMP_CAMBWD_CELLS_VALID), EINVAL, ERR_CELLS)
    assert not isinstance(bwd(tiny, A.VAMP_CAMBWD_CELLS_VALID | A.VAMP_CAMBWD_PART_GATHER), tuple)   # (no per-ray part)
    refused(bwd(tiny, A.VAMP_CAMBWD_ACCUMULATE, geom=1), EINVAL, ERR_SPLAT)
    refused(bwd(tiny, A.VAMP_CAMBWD_SPLAT, wait=1), EINVAL, ERR_SPLAT)
    many = case_desc(Case("tiny"))
    many.B, many.fH, many.fW = 6, 2000, 2000                    # 2.9e9 samples
    refused(bwd(many), EINVAL, ERR_COUNT)
    same_plan(bwd(many), bwd_plan(shape_numbers(many), 0, 1, 0, 0, huge), A.VampCameraBackwardPlan, "many")
    cells_valid = A.VAMP_CAMBWD_CELLS_VALID | A.VAMP_CAMBWD_TERM_VALID
    assert not isinstance(bwd(many, cells_valid), tuple)        # (the prepare pass's limit, where it does not run)
    deep = case_desc(Case("tiny"))
    deep.D = 202
    refused(bwd(deep), EINVAL, ERR_LDS)
    deep.D = 201
    assert bwd(deep).ray_lds == 150 * 1024 and bwd(deep).raise_lds == 1
    wide = case_desc(Case("tiny"))
    wide.B, wide.Z, wide.Y, wide.X = 33, 510, 2046, 2046        # 2.2e9 x-runs
    refused(bwd(wide, cells_valid), EINVAL, ERR_RUNS)
    refused(bwd(wide, A.VAMP_CAMBWD_PART_HEAVY), EINVAL, ERR_RUNS)
    refused(bwd(wide), EINVAL, ERR_COUNT)                       # (the earlier refusal of a whole call)
    assert not isinstance(bwd(wide, cells_valid | A.VAMP_CAMBWD_PART_RAY), tuple)
    for d_, name in ((many, "many"), (deep, "deep"), (wide, "wide")):
        nn = shape_numbers(d_)
        for f in (0, cells_valid, A.VAMP_CAMBWD_PART_HEAVY, cells_valid | A.VAMP_CAMBWD_PART_RAY, A.VAMP_CAMBWD_SPLAT):
            same_plan(bwd(d_, f), bwd_plan(nn, 0, 1, f, 0, huge), A.VampCameraBackwardPlan, (name, f))
    fwd = ask(lib.vamp_render_camera_forward_plan, A.VampCameraForwardPlan, C.byref(tiny), 0, A.VAMP_CAMFWD_SAVE_SAMPLES, n["rows"] - 1)
    refused(fwd, ENOSPC, f"vamp_render_camera_forward_plan: workspace {n['rows'] - 1} < {n['rows']} bytes")
    # a NULL descriptor or plan is refused, not read
    assert lib.vamp_render_camera_forward_plan(None, 0, 0, 0, C.byref(A.VampCameraForwardPlan())) == EINVAL
    assert lib.vamp_last_error().decode().endswith("desc is NULL")
    assert lib.vamp_render_camera_forward_plan(C.byref(tiny), 0, 0, 0, None) == EINVAL
    assert lib.vamp_last_error().decode().endswith("plan is NULL")
    assert lib.vamp_render_camera_backward_plan(None, 0, 1, 0, 0, 0, C.byref(A.VampCameraBackwardPlan())) == EINVAL
    assert lib.vamp_last_error().decode().endswith("desc is NULL")
    assert lib.vamp_render_camera_backward_plan(C.byref(tiny), 0, 1, 0, 0, 0, None) == EINVAL
    assert lib.vamp_last_error().decode().endswith("plan is NULL")


# ---------------------------------------------------------------------------------------------------- CPU: coverage
def test_sweep_reaches_every_compiled_body():
    """Every compiled camera-forward (NCH x ERT on / off x f32 / bf16), merged-launch (NCH x f32 / bf16, planned only),
    march / cell-backward (CP, planned and unplanned) and per-ray-backward ((CP / 4, KT)) body is reached by at least
    one oracle-compared case: the bodies are those the library's own plans name for the case's descriptor.  Adding a
    body to a launcher means adding it here and a case that reaches it."""
    lib, A = library(), _capi
    nch_bodies = {8, 12, 21, 24, 32}
    cp_bodies = {12, 24, 32}
    ray_bodies = {(3, 0), (6, 18), (6, 0), (8, 0)}

    def forward(c, flags):
        p = ask(lib.vamp_render_camera_forward_plan, A.VampCameraForwardPlan, C.byref(case_desc(c)), 0, flags, 1 << 62)
        assert (p.path != A.VAMP_CAMPLAN_FWD_MARCH) == planned(c.S), c.name
        return p

    def backward(c):
        return ask(lib.vamp_render_camera_backward_plan, A.VampCameraBackwardPlan, C.byref(case_desc(c)), 0, 1, 0, 0, 1 << 62)
    # the one-kernel forward (with and without termination) and the merged forward run on every planned case, in the
    # case's volume dtype
    direct = {(forward(c, A.VAMP_CAMFWD_DIRECT | (0 if p["ert"] else A.VAMP_CAMFWD_NO_ERT)).body, c.bf16, p["ert"])
              for c in CASES if planned(c.S) for p in PATHS.values() if p["cam_direct"]}
    assert direct == {(n, dt, e) for n in nch_bodies for dt in (False, True) for e in (False, True)}, sorted(direct)
    merged = {(forward(c, A.VAMP_CAMFWD_DIRECT).body, c.bf16) for c in CASES if planned(c.S)
              for p in PATHS.values() if p["cam_direct"] and p["ert"] and p["fwd_merged"]}
    assert merged == {(n, dt) for n in nch_bodies for dt in (False, True)}, sorted(merged)
    assert all(forward(c, A.VAMP_CAMFWD_DIRECT).path == A.VAMP_CAMPLAN_FWD_DIRECT for c in CASES if planned(c.S))
    # planned march / planned cell backward, and their unplanned forms above kPlanMax, at every CP
    assert {(4 * forward(c, 0).body, planned(c.S)) for c in CASES} >= {(cp, p) for cp in cp_bodies for p in (True, False)}
    assert {(backward(c).ray_cp4, backward(c).ray_kt) for c in CASES} == ray_bodies
    for K in CLASSES:                                          # every class count with cat_seg off and on
        assert {c.cat_seg for c in CASES if c.K == K and c.S == 20 and not c.bf16} == {False, True}, K
    # the plan's word split (64, 128), the per-wave split below NW = 4, and both sides of kPlanMax
    depths = {c.S for c in CASES}
    assert {1, 2, 3, 63, 64, 65, 127, 128, 129} <= depths
    assert any(planned(S) for S in depths) and any(not planned(S) for S in depths)
    assert any(c.final_dim[0] // 4 % 8 and c.final_dim[1] // 4 % 8 for c in CASES)
    assert {0, 64} <= {c.C for c in CASES}
    assert {D for D in LIFT_DEPTHS if D > PLAN_MAX} and {D for D in LIFT_DEPTHS if D <= PLAN_MAX}


# the C++ the mirrors above copy: if one of these lines changes, the mirror (and the coverage table) needs a look
DISPATCH_SOURCE = {
    "render_cam_direct.hip": ["if (nch <= 8) VAMP_CAMD(T, 8);", "else if (nch <= 12) VAMP_CAMD(T, 12);",
                              "else if (nch == 21) VAMP_CAMD(T, 21);", "else if (nch <= 24) VAMP_CAMD(T, 24);",
                              "else VAMP_CAMD(T, 32);"],
    "render_fwd_merged.hip": ["const int S = P.D - 1, nch = cam_direct_nch(P.K + 3);", "if (nch == 8) VAMP_MRG(T, 8);",
                              "else if (nch == 12) VAMP_MRG(T, 12);", "else if (nch == 21) VAMP_MRG(T, 21);",
                              "else if (nch == 24) VAMP_MRG(T, 24);", "else VAMP_MRG(T, 32);",
                              "return d->D - 1 <= kPlanMax && bev_fwd_fused_supported(d)"],
    "render_common.hpp": ["const int need = 1 + d->K + 3;", "p.CP = need <= 12 ? 12 : (need <= 24 ? 24 : 32);",
                          "inline int cam_direct_nch(int nch) { return nch <= 8 ? 8 : (nch <= 12 ? 12 : "
                          "(nch == 21 ? 21 : (nch <= 24 ? 24 : 32))); }"],
    # (the marches', the cell backward's and the per-ray pass's dispatch is compared by value:
    # test_camera_plans_are_the_mirrors)
    "ray_plan.hpp": ["constexpr int kPlanMax = 128;"],
}


def test_dispatch_mirrors():
    """The mirrors above hold for the sweep's class counts (K = 18 is the exact NCH = 21 instance, K = 17 pads 20
    channels to 24, K = 21 needs 25 packed channels), and the launcher lines they copy are still those of the source
    (DISPATCH_SOURCE): a change to the dispatch fails here until the mirrors are brought along."""
    import os
    from conftest import ROOT
    for fname, lines in DISPATCH_SOURCE.items():
        text = " ".join(open(os.path.join(ROOT, "vampire_amd", "csrc", fname)).read().split())
        for line in lines:
            assert " ".join(line.split()) in text, f"{fname}: dispatch line changed: {line}"
    assert [cam_direct_nch(K) for K in CLASSES] == [8, 8, 12, 12, 24, 21, 24, 24, 32, 32]
    assert [channel_pack(K) for K in CLASSES] == [12, 12, 12, 24, 24, 24, 24, 32, 32, 32]
    assert ray_body(18) == (6, 18) and ray_body(17) == (6, 0) and ray_body(20) == (6, 0) and ray_body(21) == (8, 0)
    for S in DEPTHS:
        lo, hi, step = depth_bound(S)
        cfg = dataclasses.replace(CFG_TINY, d_bound=(lo, hi, step))
        assert cfg.D == S + 1 and 8.0 <= hi <= 14.0, (S, hi)
