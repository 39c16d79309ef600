"""The render and lift kernels across the shape values that pick their compiled bodies and code paths -- the depth-bin
count S = D - 1, the class count K, the mid-channel count C, a ragged frustum and bf16 volumes -- against the oracle
evaluated in float64 (oracle/aten_oracle.py, compute_dtype): every output and every gradient, on each forced path.

One axis moves at a time from CFG_TINY (B = 2, six cameras).  The scene is the sdf workload with the low-x half of the
density volume turned into the "empty" regime (as tests/test_deep_tiles.py does), so rays that saturate within a few
samples share tiles with rays that run to the last depth index.

Bars are relative to the largest magnitude of the reference tensor and were set from the measured errors (at most ten
times the largest error seen over the sweep, never above the 1e-4 of the north star).  The CPU tests at the end map the
sweep's parameter lists through mirrors of the launchers' dispatch and fail if a compiled body is reached by no case.
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
    """render_bwd_ray.hip: the per-ray backward's (CP / 4, KT) instance."""
    cp = channel_pack(K)
    return (cp // 4, 18 if (cp == 24 and K == 18) else 0)


def planned(S):
    return S <= PLAN_MAX


# ---------------------------------------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def scene(case):
    """CPU tensors: (cfg, render_mats [B,N,3,4,4], volumes (fp32, bf16-rounded for bf16 cases), beta)."""
    cfg = case.cfg
    s2e, intrin, ida = synthetic.camera_rig(cfg, 2, jitter=1.0, seed=5)
    bda = synthetic.bda_matrix(2, rot_deg=5.0)
    rm = render_matrices(s2e, intrin, ida, bda)
    vols = list(synthetic.render_inputs(cfg, 2, seed=17))
    d = vols[0].clone()
    d[..., : d.shape[-1] // 2] *= 0.4         # the "empty" regime: s - bias ~ +0.6, sigma ~ 0.012 / m
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


def check_path(case, path, calls):
    """The calls that ran are those of the path the case asked for (or, above kPlanMax, of its documented fallback)."""
    S = case.S
    p = PATHS[path]
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
        assert bool(fwd[1] & _capi.VAMP_CAMFWD_SAVE_SAMPLES) == p["save_rows"], fwd
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


# ---------------------------------------------------------------------------------------------------- CPU: coverage
def test_sweep_reaches_every_compiled_body():
    """Every compiled camera-forward (NCH x ERT on / off x f32 / bf16), merged-launch (NCH x f32 / bf16, planned only),
    march / cell-backward (CP, planned and unplanned) and per-ray-backward ((CP / 4, KT)) body is reached by at least
    one oracle-compared case.  Adding a body to a launcher means adding it here and a case that reaches it."""
    nch_bodies = {8, 12, 21, 24, 32}
    cp_bodies = {12, 24, 32}
    ray_bodies = {(3, 0), (6, 18), (6, 0), (8, 0)}
    # the one-kernel forward (with and without termination) and the merged forward run on every planned case, in the
    # case's volume dtype
    direct = {(cam_direct_nch(c.K), c.bf16, p["ert"]) for c in CASES if planned(c.S)
              for p in PATHS.values() if p["cam_direct"]}
    assert direct == {(n, dt, e) for n in nch_bodies for dt in (False, True) for e in (False, True)}, sorted(direct)
    merged = {(cam_direct_nch(c.K), c.bf16) for c in CASES if planned(c.S)
              for p in PATHS.values() if p["cam_direct"] and p["ert"] and p["fwd_merged"]}
    assert merged == {(n, dt) for n in nch_bodies for dt in (False, True)}, sorted(merged)
    # planned march / planned cell backward, and their unplanned forms above kPlanMax, at every CP
    assert {(channel_pack(c.K), planned(c.S)) for c in CASES} >= {(cp, p) for cp in cp_bodies for p in (True, False)}
    assert {ray_body(c.K) for c in CASES} == ray_bodies
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
    "render_cam_direct_dev.hpp": ["inline int cam_direct_nch(int nch) { return nch <= 8 ? 8 : (nch <= 12 ? 12 : "
                                  "(nch == 21 ? 21 : (nch <= 24 ? 24 : 32))); }"],
    "render_cam_direct.hip": ["if (nch <= 8) VAMP_CAMD(T, 8);", "else if (nch <= 12) VAMP_CAMD(T, 12);",
                              "else if (nch == 21) VAMP_CAMD(T, 21);", "else if (nch <= 24) VAMP_CAMD(T, 24);",
                              "else VAMP_CAMD(T, 32);"],
    "render_fwd_merged.hip": ["const int S = P.D - 1, nch = cam_direct_nch(P.K + 3);", "if (nch == 8) VAMP_MRG(T, 8);",
                              "else if (nch == 12) VAMP_MRG(T, 12);", "else if (nch == 21) VAMP_MRG(T, 21);",
                              "else if (nch == 24) VAMP_MRG(T, 24);", "else VAMP_MRG(T, 32);",
                              "return d->D - 1 <= kPlanMax && bev_fwd_fused_supported(d)"],
    "render_common.hpp": ["const int need = 1 + d->K + 3;", "p.CP = need <= 12 ? 12 : (need <= 24 ? 24 : 32);"],
    "render_bwd_ray.hip": ["if (P.CP == 12) VAMP_RAY(3, 0); else if (P.CP == 24 && P.K == 18) VAMP_RAY(6, 18); "
                           "else if (P.CP == 24) VAMP_RAY(6, 0); else VAMP_RAY(8, 0);"],
    "render_bwd_cell.hip": ["const bool planned = S <= kPlanMax;",
                            "if (P.CP == 12) VAMP_CELL(3, 2); else if (P.CP == 24) VAMP_CELL(6, VAMP_SPLAT_NW); "
                            "else VAMP_CELL(8, 4);"],
    "render_fwd.hip": ["const bool planned = !geom && d->D - 1 <= kPlanMax;",
                       "if (P.CP == 12) VAMP_CAMP(3); else if (P.CP == 24) VAMP_CAMP(6); else VAMP_CAMP(8);",
                       "if (P.CP == 12) VAMP_CAM(3); else if (P.CP == 24) VAMP_CAM(6); else VAMP_CAM(8);"],
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
