"""cfg-B camera tiles whose rays never saturate next to tiles whose rays do: the scan of the one-kernel camera forward
(cam_fwd_direct_tile) then runs over every depth bin of some rays and over a few of others, in one workgroup."""
import ctypes as C
import json
import os

import pytest
import torch

from conftest import GOLDEN
from vampire_amd.config import CFG_B
from vampire_amd import _capi
from test_hip_parity import NAMES, close, hot, _regime_inputs, _render_fwd_bwd, _upstream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def scene(dev):
    """The synthetic sdf workload with the low-x half of the density volume turned into the "empty" regime
    (s - bias ~ +0.6: sigma ~ 0.012 / m, no ray crossing only that half saturates)."""
    with open(os.path.join(GOLDEN, "full_checksums.json")) as f:
        rm = torch.tensor(json.load(f)["B"]["render_mats"], dtype=torch.float32, device=dev)
    cfg, vols = _regime_inputs(CFG_B, "sdf", dev, with_grad=False)
    d = vols[0].clone()
    X = d.shape[-1]
    d[..., : X // 2] *= 0.4
    vols[0] = d
    return cfg, [v.detach().requires_grad_(True) for v in vols], rm


def _term(hp, cfg, B=1):
    """The termination table the last render call of `hp` left in its workspace: [B * N, fH, fW]."""
    d = hp.render_desc(B, cfg.num_cams, _capi.VAMP_F32)
    off = hp.lib.vamp_render_term_offset(C.byref(d))
    n = B * cfg.num_cams * cfg.fH * cfg.fW
    return hp._ws["render"][off:off + 4 * n].view(torch.int32).clone().view(B * cfg.num_cams, cfg.fH, cfg.fW)


def _forward(cfg, vols, rm, dev, merged):
    hp = hot(cfg, dev)
    hp.impl.update(cam_direct=True, ert=True, fwd_merged=merged)
    with torch.no_grad():
        outs = hp.render(*[v.detach() for v in vols], torch.tensor(0.1, device=dev), render_mats=rm)
    return [o.clone() for o in outs], _term(hp, cfg)


def test_scene_mixes_deep_and_shallow_rays_in_tiles(dev, scene):
    """The fixture does what the other tests rely on: tiles holding both rays that run to the last depth index and
    rays that stop early, and rays that never saturate at all."""
    cfg, vols, rm = scene
    _, term = _forward(cfg, vols, rm, dev, True)
    S = cfg.D - 1
    t = term.view(cfg.num_cams, cfg.fH // 8, 8, cfg.fW // 8, 8).permute(0, 1, 3, 2, 4).reshape(-1, 64)
    deep = (t == S).sum(dim=1)
    assert int((t == S).sum()) > 0 and int((t < S).sum()) > 0
    mixed = (deep > 0) & (deep < 64)
    assert int(mixed.sum()) >= 8, f"only {int(mixed.sum())} tiles mix deep and shallow rays"
    assert int(((deep > 0) & (deep <= 4)).sum()) > 0, "no tile with a handful of survivors"


def test_deep_tiles_termination_on_equals_off(dev, scene):
    """Outputs and gradients with early termination against the termination-off path, at the tolerances of
    test_ert_on_equals_off_full_size."""
    cfg, vols, rm = scene
    on = _render_fwd_bwd(cfg, vols, rm, dev, True, 4545, cam_direct=True)
    off = _render_fwd_bwd(cfg, vols, rm, dev, False, 4545, cam_direct=True)
    for nm, a, b in zip(NAMES, on[0], off[0]):
        close(a, b, atol=(3 * 1.2e-7 * cfg.d_bound[1] if nm == "depth_preds" else 1e-7), rtol=1e-6, scale="max",
              what=f"deep tiles ERT on/off {nm}")
    for nm, a, b in zip(("density_feature", "semantic_logits", "base", "rgb"), on[1], off[1]):
        close(a, b, atol=1e-12, rtol=1e-5, scale="max", what=f"deep tiles ERT on/off grad_{nm}")
    assert abs(float(on[2]) - float(off[2])) <= 1e-5 * abs(float(off[2])) + 1e-9, (float(on[2]), float(off[2]))


def test_deep_tiles_merged_equals_two_launches(dev, scene):
    """The merged render forward against the stand-alone camera kernel + BEV launch: outputs and termination table
    bit for bit."""
    cfg, vols, rm = scene
    m_outs, m_term = _forward(cfg, vols, rm, dev, True)
    s_outs, s_term = _forward(cfg, vols, rm, dev, False)
    for nm, a, b in zip(NAMES, m_outs, s_outs):
        assert torch.equal(a, b), f"merged launch differs from the two launches in {nm}"
    assert torch.equal(m_term, s_term), "termination table"


def test_deep_tiles_same_bits_twice(dev, scene):
    """Two training calls on the same inputs: identical outputs and termination table.  (The gradients are fp32 sums in
    the order the backward's atomics hand out slots, which moves their last bits from run to run: they are held to the
    tolerance of test_ert_on_equals_off_full_size.)"""
    cfg, vols, rm = scene
    runs = []
    for _ in range(2):
        hp = hot(cfg, dev)
        hp.impl.update(cam_direct=True, ert=True)
        for v in vols:
            v.grad = None
        beta = torch.tensor(0.1, device=dev, requires_grad=True)
        outs = hp.render(*vols, beta, render_mats=rm)
        term = _term(hp, cfg)
        torch.autograd.backward(outs, _upstream([o.shape for o in outs], 4545, dev))
        runs.append(([o.detach().clone() for o in outs], term, [v.grad.clone() for v in vols], beta.grad.clone()))
    (oa, ta, ga, ba), (ob, tb, gb, bb) = runs
    for nm, x, y in zip(NAMES, oa, ob):
        assert torch.equal(x, y), f"output {nm} differs between two runs"
    assert torch.equal(ta, tb), "termination table differs between two runs"
    for nm, x, y in zip(("density_feature", "semantic_logits", "base", "rgb"), ga, gb):
        close(x, y, atol=1e-12, rtol=1e-5, scale="max", what=f"grad_{nm} between two runs")
    assert abs(float(ba) - float(bb)) <= 1e-5 * abs(float(bb)) + 1e-9, (float(ba), float(bb))
