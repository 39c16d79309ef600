"""The contract between a caller's tensor and the kernels' raw pointers: every public operator of the hot path gives
the same values for the same numbers in any memory layout -- strided views, permuted memory, views at an odd offset,
expanded tensors, upstream gradients that are none of contiguous / fp32 / defined, fp16 and fp64 inputs -- and refuses a
wrong shape, a host tensor or an integer volume from Python, before any library call.

Every HotPath of this file runs under tests/call_guard.py: a tensor that reaches the library strided, short, on the
wrong device or with the wrong element size ends the test with ContractViolation instead of a launch.

Bars.  Forward outputs are bit-deterministic (test_deep_tiles_same_bits_twice): torch.equal against the contiguous run.
Input gradients are fp32 sums in the order the backward's atomics hand out slots: they are held to what
tests/test_deep_tiles.py allows between two runs of the SAME input, close(atol=1e-12, rtol=1e-5, scale="max") and the
1e-5 relative rule for grad_beta.  A wrong stride scrambles values at order one.  A 16-bit input gets its gradient in
its own dtype: the fp32 result rounded once, so the bar is that rounding (2^-8 of the largest magnitude for bf16, as
test_render_shape_sweep.BF16_GRAD_REL; 2^-11 for fp16's 11-bit significand) on top of the two-run bar."""
import copy
import functools

import pytest
import torch

import call_guard
from call_guard import ContractViolation
from vampire_amd import _capi, backbone, synthetic
from vampire_amd.config import CFG_TINY
from test_hip_parity import NAMES, channel_last, close, hot, _upstream
import test_render_shape_sweep as RS
from test_hot_path_sequences import RCase, lift_seq_scene

pytestmark = pytest.mark.gpu

B = 2
RUN_RTOL, RUN_ATOL = 1e-5, 1e-12               # two runs of the same input (tests/test_deep_tiles.py)
ROUNDING = {torch.bfloat16: RS.BF16_GRAD_REL, torch.float16: 2.0 ** -11, torch.float64: 0.0, torch.float32: 0.0}
REFUSALS = (ValueError, TypeError, _capi.VampireHipError)
PLANNED = "planned-ert"                        # one of the planned paths of RS.PATHS beside the default ("auto")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------- the same values, other memory
def v_strided(x):
    """A step-2 slice along the leading and along the innermost axis of a larger tensor."""
    if x.dim() == 0:
        return torch.zeros(2, dtype=x.dtype, device=x.device)[::2].copy_(x.reshape(1)).reshape(())
    shape = list(x.shape)
    shape[0] *= 2
    shape[-1] *= 2 if x.dim() > 1 else 1
    big = torch.full(shape, 7.0, device=x.device).to(x.dtype)
    view = big[::2, ..., ::2] if x.dim() > 1 else big[::2]
    view.copy_(x)
    assert view.shape == x.shape and (not view.is_contiguous() or x.numel() <= 1)
    return view


def v_permuted(x, i=-1, j=-2):
    """x.transpose(i, j).contiguous().transpose(i, j): the same tensor over permuted memory."""
    out = x.transpose(i, j).contiguous().transpose(i, j)
    assert out.shape == x.shape
    return out


def v_offset(x):
    """A contiguous view that starts one element into a larger buffer (4 or 2 bytes past the allocator's alignment)."""
    buf = torch.zeros(x.numel() + 1, dtype=x.dtype, device=x.device)
    view = buf[1:].view(x.shape).copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    return view


VARIANTS = {"strided": v_strided, "permuted": v_permuted, "offset": v_offset}


def variants_of(x, extra=None):
    out = {k: f for k, f in VARIANTS.items() if not (k == "permuted" and (x.dim() < 2 or x.shape[-1] * x.shape[-2] == 1))}
    out.update(extra or {})
    return out


# ---------------------------------------------------------------------------------------------------- one guarded call
def guarded(cfg, dev, impl=None):
    hp = hot(cfg, dev)
    hp.impl.update(impl or {})
    return hp, call_guard.install(hp)


def run(cfg, dev, call, inputs, grads=(), upstream=None, impl=None, only=None):
    """`call(hp, **inputs)` on a fresh guarded HotPath: (outputs, {input: gradient}).  The inputs named in `grads` become
    leaves AS THEY ARE (detach() keeps strides and offset); `upstream(outs)` gives the incoming gradients (seeded
    noise by default); `only`: the indices of the outputs that get one (the others stay undefined)."""
    hp, guard = guarded(cfg, dev, impl)
    leaves = {k: (v.detach().requires_grad_(True) if k in grads else v) for k, v in inputs.items()}
    for k in grads:
        assert leaves[k].stride() == inputs[k].stride() and leaves[k].data_ptr() == inputs[k].data_ptr()
    outs = call(hp, **leaves)
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    got = {}
    if grads:
        ups = upstream(outs) if upstream is not None else _upstream([o.shape for o in outs], 4545, dev)
        if callable(ups):
            ups()                                            # (the upstream is an expression on the outputs)
        else:
            idx = range(len(outs)) if only is None else only
            torch.autograd.backward([outs[i] for i in idx], [ups[i] for i in idx])
        for k in grads:
            g = leaves[k].grad
            assert g is not None, f"no gradient for {k}"
            assert g.shape == leaves[k].shape, f"grad {k}: shape {tuple(g.shape)} for an input {tuple(leaves[k].shape)}"
            assert g.dtype == leaves[k].dtype, f"grad {k}: {g.dtype} for a {leaves[k].dtype} input"
            got[k] = g
    assert guard.log, "the call did not go through the guard"
    return [o.detach() for o in outs], got


def same(got, ref, what, rounding=None):
    """Outputs bit for bit, gradients at the two-run bar (plus one rounding of a 16-bit gradient's dtype)."""
    (go, gg), (ro, rg) = got, ref
    assert len(go) == len(ro)
    for i, (a, b) in enumerate(zip(go, ro)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: output {i} {tuple(a.shape)} {a.dtype}"
        assert torch.equal(a, b), f"{what}: output {i} differs, max |diff| {float((a.double() - b.double()).abs().max()):.3e}"
    assert set(gg) == set(rg)
    for k in rg:
        a, b = gg[k].detach().double().cpu(), rg[k].detach().double().cpu()
        top = max(float(b.abs().max()), 1e-30)
        err = float((a - b).abs().max()) / top
        extra = (rounding or {}).get(k, 0.0)
        print(f"{what}: grad_{k} err {err:.3e} of max |ref| {top:.3e} (bar {RUN_RTOL + extra:.3e})")
        if k == "beta":
            assert abs(float(a) - float(b)) <= RUN_RTOL * abs(float(b)) + 1e-9, (what, float(a), float(b))
        elif extra:
            lim = RUN_ATOL + (RUN_RTOL + extra) * top
            assert float((a - b).abs().max()) <= lim, f"{what}: grad_{k} err {err:.3e} of max (bar {RUN_RTOL + extra:.3e})"
        else:
            close(a, b, atol=RUN_ATOL, rtol=RUN_RTOL, scale="max", what=f"{what}: grad_{k}")


def sweep(cfg, dev, call, inputs, grads, what, upstream=None, impl=None, extra=None, skip=()):
    """The contiguous, aligned run against every variant of every tensor input, one input at a time; returns what ran."""
    ref = run(cfg, dev, call, inputs, grads, upstream, impl)
    again = run(cfg, dev, call, inputs, grads, upstream, impl)
    same(again, ref, f"{what}: two runs")
    ran = []
    for name, x in inputs.items():
        if not isinstance(x, torch.Tensor) or name in skip:
            continue
        for vname, fn in variants_of(x, (extra or {}).get(name)).items():
            v = fn(x)
            assert v.numel() == x.numel() and (v.shape == x.shape or x.dim() == 0) and torch.equal(v.reshape(x.shape), x), \
                (name, vname)
            same(run(cfg, dev, call, dict(inputs, **{name: v}), grads, upstream, impl), ref, f"{what}: {name} {vname}")
            ran.append(f"{name}/{vname}")
    print(f"RAN {what}: " + " ".join(ran))
    return ref


def refusals(cfg, dev, cases):
    """Every (what, thunk(hp)) raises from Python and no library call is made: the guard's log stays empty."""
    hp, guard = guarded(cfg, dev)
    for what, thunk in cases:
        try:
            with pytest.raises(REFUSALS):
                thunk(hp)
        except ContractViolation as v:
            pytest.fail(f"{what}: reached the library -- {v}")
        assert guard.log == [], f"{what}: {[n for n, _ in guard.log]} ran"
    print("REFUSED " + ", ".join(w for w, _ in cases))


def grown(x, axis, by=1):
    """x with one axis longer (by > 0) or shorter: a wrong-shaped tensor of the same kind."""
    shape = list(x.shape)
    shape[axis] += by
    return torch.zeros(shape, dtype=x.dtype, device=x.device)


# ---------------------------------------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def lift_scene(dev):
    cfg, geo, lm, depth, feat, gout = lift_seq_scene(B, 4)            # the smallest channel count of the lift scenes
    return cfg, dict(depth=depth.to(dev), feat=feat.to(dev), lift_mats=lm.to(dev)), gout.to(dev)


@functools.lru_cache(maxsize=None)
def render_scene(dev):
    cfg, rm, vols, beta_v = RS.scene(RCase("tiny", B=B))
    dens, sem, base, rgb = (v.to(dev) for v in vols)
    ins = dict(density_feature=dens, semantic_logits=sem, base=base, rgb=rgb, beta=torch.tensor(beta_v, device=dev),
               render_mats=rm.to(dev))
    return cfg, ins


def render_call(hp, density_feature, semantic_logits, base, rgb, beta, render_mats=None, geom=None):
    return hp.render(density_feature, semantic_logits, base, rgb, beta, render_mats=render_mats, geom=geom)


RENDER_GRADS = ("density_feature", "semantic_logits", "base", "rgb", "beta")


@functools.lru_cache(maxsize=None)
def points_scene(dev):
    cfg, ins = render_scene(dev)
    gen = torch.Generator().manual_seed(31)
    span = torch.tensor([b[1] - b[0] for b in (cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg)])
    lo = torch.tensor([b[0] for b in (cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg)])
    pts = lo + span * (torch.rand(B, 77, 3, generator=gen) * 1.2 - 0.1)       # a tenth of the points outside each face
    return cfg, ins, pts.to(dev)


def expanded_beta(x):
    """One element of an expanded tensor (stride 0)."""
    v = x.reshape(1).expand(4)[1:2]
    assert v.stride() == (0,)
    return v


# ---------------------------------------------------------------------------------------------------- layout sweeps
@pytest.mark.parametrize("op", ["lift", "lift-d1", "lift_logits", "lift_dense"])
def test_lift_layouts(dev, op):
    cfg, ins, gout = lift_scene(dev)
    ups = lambda outs: [gout]
    if op == "lift":
        sweep(cfg, dev, lambda hp, **k: hp.lift(**k), ins, ("depth", "feat"), "lift", ups,
              extra={"feat": {"channel-last": channel_last}})
        # (d) matrices shared by the samples, one expanded [1, N, 3, 4, 4]; a depth constant over the planes
        shared = dict(ins, lift_mats=ins["lift_mats"][:1].expand_as(ins["lift_mats"]).contiguous(),
                      depth=torch.full_like(ins["depth"][:, :, :1], 1.0 / cfg.D).expand_as(ins["depth"]).contiguous())
        ref = run(cfg, dev, lambda hp, **k: hp.lift(**k), shared, ("depth", "feat"), ups)
        for name, fn in (("lift_mats", lambda m: m[:1].expand_as(m)),
                         ("depth", lambda d: d[:, :, :1].expand_as(d))):
            v = fn(shared[name])
            assert torch.equal(v, shared[name]) and 0 in v.stride()
            same(run(cfg, dev, lambda hp, **k: hp.lift(**k), dict(shared, **{name: v}), ("depth", "feat"), ups), ref,
                 f"lift: {name} expanded")
    elif op == "lift-d1":
        d1 = dict(depth=None, feat=ins["feat"], lift_mats=ins["lift_mats"])
        sweep(cfg, dev, lambda hp, **k: hp.lift(use_depth=False, **k), d1, ("feat",), "lift use_depth=False", ups,
              extra={"feat": {"channel-last": channel_last}})
    elif op == "lift_logits":
        lg = dict(logits=ins["depth"].clamp_min(1e-30).log(), feat=ins["feat"], lift_mats=ins["lift_mats"])
        sweep(cfg, dev, lambda hp, **k: hp.lift_logits(**k), lg, ("logits", "feat"), "lift_logits", ups,
              extra={"feat": {"channel-last": channel_last}})
    else:
        ff = (ins["depth"].unsqueeze(2) * ins["feat"].unsqueeze(3)).contiguous()
        sweep(cfg, dev, lambda hp, **k: hp.lift_dense(**k), dict(frustum_feats=ff, lift_mats=ins["lift_mats"]),
              ("frustum_feats",), "lift_dense", ups)


@pytest.mark.parametrize("path", ["default", PLANNED])
@pytest.mark.parametrize("geometry", ["render_mats", "geom"])
def test_render_layouts(dev, path, geometry):
    cfg, ins = render_scene(dev)
    impl = None if path == "default" else RS.PATHS[path]
    if geometry == "geom":
        hp, _ = guarded(cfg, dev)
        ins = dict({k: v for k, v in ins.items() if k != "render_mats"}, geom=hp.frustum_geometry(ins["render_mats"]))
    extra = {"beta": {"expanded": expanded_beta}}
    sweep(cfg, dev, render_call, ins, RENDER_GRADS, f"render[{path}, {geometry}]", impl=impl, extra=extra)
    # (d) a volume that is one plane repeated along z, and matrices shared by the samples
    const = dict(ins, rgb=ins["rgb"][:, :, :1].expand_as(ins["rgb"]).contiguous())
    variants = [("rgb", lambda r: r[:, :, :1].expand_as(r))]
    if geometry == "render_mats":
        const["render_mats"] = ins["render_mats"][:1].expand_as(ins["render_mats"]).contiguous()
        variants.append(("render_mats", lambda m: m[:1].expand_as(m)))
    ref = run(cfg, dev, render_call, const, RENDER_GRADS, impl=impl)
    for name, fn in variants:
        v = fn(const[name])
        assert torch.equal(v, const[name]) and 0 in v.stride()
        same(run(cfg, dev, render_call, dict(const, **{name: v}), RENDER_GRADS, impl=impl), ref,
             f"render[{path}, {geometry}]: {name} expanded")


@pytest.mark.parametrize("padding", ["zeros", "border"])
@pytest.mark.parametrize("channel_last_out", [False, True], ids=["cf", "cl"])
def test_sample_points_layouts(dev, padding, channel_last_out):
    cfg, ins, pts = points_scene(dev)
    call = lambda hp, volume, points: hp.sample_points(volume, points, padding=padding, channel_last=channel_last_out,
                                                       mask_outside=(padding == "zeros"))
    sweep(cfg, dev, call, dict(volume=ins["semantic_logits"], points=pts), ("volume",),
          f"sample_points[{padding}, {'cl' if channel_last_out else 'cf'}]")
    if padding != "zeros":
        return
    # the activated density as the reference samples it (bv2:604: zeros padding; beta read, grad_beta returned)
    act = lambda hp, volume, points, beta: hp.sample_points(volume, points, padding=padding, activation=True, beta=beta,
                                                            channel_last=channel_last_out)
    sweep(cfg, dev, act, dict(volume=ins["density_feature"], points=pts, beta=ins["beta"]), ("volume", "beta"),
          f"sample_points[{padding}, {'cl' if channel_last_out else 'cf'}, activation]",
          extra={"beta": {"expanded": expanded_beta}})


def test_occupancy_queries_layouts(dev):
    cfg, ins, _ = points_scene(dev)
    ax = [torch.linspace(b[0] * 1.05, b[1] * 1.05, n) for b, n in zip((cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg),
                                                                       (7, 5, 3))]
    occ = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).to(dev)
    bda = synthetic.bda_matrix(B, rot_deg=5.0).to(dev)
    call = lambda hp, semantic_logits, density_feature, occ_coords, bda_mat, beta: hp.occupancy_queries(
        semantic_logits, density_feature, occ_coords, bda_mat, beta)
    args = dict(semantic_logits=ins["semantic_logits"], density_feature=ins["density_feature"], occ_coords=occ, bda_mat=bda,
                beta=ins["beta"])
    sweep(cfg, dev, call, args, ("semantic_logits", "density_feature", "beta"), "occupancy_queries",
          extra={"beta": {"expanded": expanded_beta}})
    sweep(cfg, dev, call, dict(args, bda_mat=None), ("semantic_logits", "density_feature", "beta"),
          "occupancy_queries[static grid]", skip=("semantic_logits", "density_feature", "beta"))


def test_glue_layouts(dev):
    cfg, ins, _ = lift_scene(dev)
    gen = torch.Generator().manual_seed(77)
    lg = (torch.randn(B * cfg.num_cams, cfg.D, cfg.fH, cfg.fW, generator=gen) * 2).to(dev)
    sweep(cfg, dev, lambda hp, logits: hp.depth_softmax(logits), dict(logits=lg), ("logits",), "depth_softmax")
    C_, cout = 4, 8
    vo = torch.randn(B, C_, cfg.oZ, cfg.oY, cfg.oX, generator=gen).to(dev)
    vd = torch.randn(B, 1, cfg.oZ, cfg.oY, cfg.oX, generator=gen).to(dev)
    sweep(cfg, dev, lambda hp, **k: hp.density_gate(**k), dict(voxel_output=vo, voxel_density=vd),
          ("voxel_output", "voxel_density"), "density_gate")
    w = (torch.randn(cout, C_ * cfg.oZ, 1, 1, generator=gen) * 0.3).to(dev)
    b = torch.randn(cout, generator=gen).to(dev)
    hp, _ = guarded(cfg, dev)
    assert hp.gate_conv1x1_supported(C_, cfg.oZ, cout)
    sweep(cfg, dev, lambda hp, **k: hp.gate_conv1x1(**k), dict(voxel_output=vo, voxel_density=vd, weight=w, bias=b),
          ("voxel_output", "voxel_density", "weight", "bias"), "gate_conv1x1",
          extra={"weight": {"permuted": lambda x: v_permuted(x, 0, 1)}})
    w2 = w.reshape(cout, -1)                                         # the weight as a matrix, no bias
    sweep(cfg, dev, lambda hp, **k: hp.gate_conv1x1(**k), dict(voxel_output=vo, voxel_density=vd, weight=w2),
          ("voxel_output", "voxel_density", "weight"), "gate_conv1x1[matrix weight, no bias]",
          skip=("voxel_output", "voxel_density"))


def test_diagnostics_layouts(dev):
    lcfg, lins, _ = lift_scene(dev)
    cfg, ins = render_scene(dev)
    lm, rm = lins["lift_mats"], ins["render_mats"]
    for ud in (True, False):
        sweep(lcfg, dev, lambda hp, lift_mats: hp.lift_indices(lift_mats, use_depth=ud), dict(lift_mats=lm), (),
              f"lift_indices[use_depth={ud}]")
        sweep(lcfg, dev, lambda hp, lift_mats: hp.lift_cull_words(lift_mats, use_depth=ud)[0], dict(lift_mats=lm), (),
              f"lift_cull_words[use_depth={ud}]")
    geom = sweep(cfg, dev, lambda hp, render_mats: hp.frustum_geometry(render_mats), dict(render_mats=rm), (),
                 "frustum_geometry")[0][0]
    sweep(cfg, dev, lambda hp, render_mats: hp.render_indices(render_mats=render_mats), dict(render_mats=rm), (),
          "render_indices[render_mats]")
    sweep(cfg, dev, lambda hp, geom: hp.render_indices(geom=geom), dict(geom=geom), (), "render_indices[geom]")
    sweep(cfg, dev, lambda hp, render_mats: hp.render_direct_taps(render_mats, coords=True), dict(render_mats=rm), (),
          "render_direct_taps")
    stats = lambda hp, density_feature, beta, render_mats: [torch.tensor(hp.ert_statistics(density_feature, beta, render_mats))]
    sweep(cfg, dev, stats, dict(density_feature=ins["density_feature"], beta=ins["beta"], render_mats=rm), (),
          "ert_statistics", extra={"beta": {"expanded": expanded_beta}})


# ---------------------------------------------------------------------------------------------------- incoming gradients
def upstream_forms(base):
    """(what, upstream to give, the contiguous fp32 upstream of the same values) per form, from contiguous fp32 `base`."""
    perm = [v_permuted(u) if u.dim() >= 2 and u.shape[-1] * u.shape[-2] > 1 else u for u in base]
    r16 = [u.bfloat16() for u in base]
    return [("permuted", perm, base), ("strided", [v_strided(u) for u in base], base),
            ("bf16", r16, [u.float() for u in r16])]


def incoming(cfg, dev, call, inputs, grads, what, base, impl=None):
    for form, ups, plain in upstream_forms(base):
        assert all(torch.equal(a.float(), b) for a, b in zip(ups, plain))
        ref = run(cfg, dev, call, inputs, grads, lambda outs: plain, impl)
        same(run(cfg, dev, call, inputs, grads, lambda outs: ups, impl), ref, f"{what}: upstream {form}")
    # expanded: out.sum().backward() against explicit ones
    ref = run(cfg, dev, call, inputs, grads, lambda outs: [torch.ones_like(o) for o in outs], impl)
    got = run(cfg, dev, call, inputs, grads, lambda outs: (lambda: sum(o.sum() for o in outs).backward()), impl)
    same(got, ref, f"{what}: upstream expanded")
    print(f"RAN {what}: upstream permuted strided bf16 expanded")


def test_lift_incoming_gradients(dev):
    cfg, ins, gout = lift_scene(dev)
    incoming(cfg, dev, lambda hp, **k: hp.lift(**k), ins, ("depth", "feat"), "lift", [gout])
    incoming(cfg, dev, lambda hp, **k: hp.lift(**k), dict(ins, feat=channel_last(ins["feat"])), ("depth", "feat"),
             "lift[channel-last feat]", [gout])


@pytest.mark.parametrize("path", ["default", PLANNED])
def test_render_incoming_gradients(dev, path):
    cfg, ins = render_scene(dev)
    impl = None if path == "default" else RS.PATHS[path]
    outs, _ = run(cfg, dev, render_call, ins, (), impl=impl)
    base = _upstream([o.shape for o in outs], 4545, dev)
    incoming(cfg, dev, render_call, ins, RENDER_GRADS, f"render[{path}]", base, impl=impl)
    # an upstream on two of the eight outputs, the others undefined: against explicit zeros
    two = (NAMES.index("rgb_preds"), NAMES.index("voxel_output"))
    zeros = [u if i in two else torch.zeros_like(u) for i, u in enumerate(base)]
    ref = run(cfg, dev, render_call, ins, RENDER_GRADS, lambda o: zeros, impl)
    same(run(cfg, dev, render_call, ins, RENDER_GRADS, lambda o: base, impl, only=two), ref,
         f"render[{path}]: upstream on two outputs")


def test_sample_points_incoming_gradients(dev):
    cfg, ins, pts = points_scene(dev)
    for cl in (False, True):
        call = lambda hp, volume, points, beta: hp.sample_points(volume, points, activation=True, beta=beta, channel_last=cl)
        args = dict(volume=ins["density_feature"], points=pts, beta=ins["beta"])
        outs, _ = run(cfg, dev, call, args)
        incoming(cfg, dev, call, args, ("volume", "beta"), f"sample_points[channel_last={cl}]",
                 _upstream([o.shape for o in outs], 4545, dev))


# ---------------------------------------------------------------------------------------------------- dtype mixes
def mixed(cfg, dev, call, inputs, grads, dtypes, what, upstream=None):
    """`inputs` with the dtypes of `dtypes` ({input: dtype}) against the run on .float() copies of the same values."""
    cast = dict(inputs, **{k: inputs[k].to(dt) for k, dt in dtypes.items()})
    plain = dict(inputs, **{k: cast[k].float() for k in dtypes})
    ref = run(cfg, dev, call, plain, grads, upstream)
    got = run(cfg, dev, call, cast, grads, upstream)          # (run() asserts each gradient has its input's dtype)
    same(got, ref, what, rounding={k: ROUNDING[dt] for k, dt in dtypes.items()})
    print(f"RAN {what}")


@pytest.mark.parametrize("dt", [torch.float16, torch.float64, torch.bfloat16], ids=["fp16", "fp64", "bf16"])
def test_lift_dtype_mixes(dev, dt):
    cfg, ins, gout = lift_scene(dev)
    call, ups = (lambda hp, **k: hp.lift(**k)), (lambda outs: [gout])
    if dt == torch.bfloat16:
        mixed(cfg, dev, call, ins, ("depth", "feat"), {"feat": dt}, "lift: fp32 depth + bf16 feat", ups)
        return
    mixed(cfg, dev, call, ins, ("depth", "feat"), {"depth": dt, "feat": dt}, f"lift: {dt} depth and feat", ups)
    mixed(cfg, dev, call, ins, ("depth", "feat"), {"depth": dt}, f"lift: {dt} depth, fp32 feat", ups)
    lg = dict(logits=ins["depth"].clamp_min(1e-30).log(), feat=ins["feat"], lift_mats=ins["lift_mats"])
    mixed(cfg, dev, lambda hp, **k: hp.lift_logits(**k), lg, ("logits", "feat"), {"logits": dt, "feat": dt},
          f"lift_logits: {dt} logits and feat", ups)


@pytest.mark.parametrize("dt", [torch.float16, torch.float64, torch.bfloat16], ids=["fp16", "fp64", "bf16"])
def test_render_and_sample_points_dtype_mixes(dev, dt):
    cfg, ins, pts = points_scene(dev)
    vols = ("density_feature", "semantic_logits", "base", "rgb")
    if dt == torch.bfloat16:
        mixed(cfg, dev, render_call, ins, RENDER_GRADS, {"rgb": dt}, "render: one bf16 volume among fp32 ones")
        return
    mixed(cfg, dev, render_call, ins, RENDER_GRADS, {k: dt for k in vols}, f"render: {dt} volumes")
    mixed(cfg, dev, lambda hp, volume, points: hp.sample_points(volume, points, padding="border"),
          dict(volume=ins["semantic_logits"], points=pts), ("volume",), {"volume": dt}, f"sample_points: {dt} volume")


# ---------------------------------------------------------------------------------------------------- mistakes raise before any launch
def _each(call, inputs, changes):
    """[(what, thunk)]: `call` with one input replaced per entry of `changes` ({what: (input, tensor)})."""
    return [(what, (lambda hp, k=k, v=v: call(hp, **dict(inputs, **{k: v})))) for what, (k, v) in changes.items()]


def _host_and_integer(inputs, integer=()):
    out = {f"{k} on the host": (k, v.cpu()) for k, v in inputs.items() if isinstance(v, torch.Tensor)}
    out.update({f"{k} int64": (k, inputs[k].long()) for k in integer})
    return out


def test_lift_mistakes_raise_before_any_launch(dev):
    cfg, ins, _ = lift_scene(dev)
    d, f, m = ins["depth"], ins["feat"], ins["lift_mats"]
    wrong = {"depth D+1": ("depth", grown(d, 2)), "depth D-1": ("depth", grown(d, 2, -1)), "depth fH+1": ("depth", grown(d, 3)),
             "depth fW-1": ("depth", grown(d, 4, -1)), "depth N-1": ("depth", grown(d, 1, -1)), "depth B+1": ("depth", grown(d, 0)),
             "feat fH+1": ("feat", grown(f, 3)), "feat fH-1": ("feat", grown(f, 3, -1)), "feat N+1": ("feat", grown(f, 1)),
             "lift_mats 4x5": ("lift_mats", grown(m, 4)), "lift_mats 2 rows": ("lift_mats", grown(m, 2, -1)),
             "lift_mats N+1": ("lift_mats", grown(m, 1))}
    wrong.update(_host_and_integer(ins, integer=("depth", "feat")))
    cases = _each(lambda hp, **k: hp.lift(**k), ins, wrong)
    lg = dict(logits=d.log(), feat=f, lift_mats=m)
    cases += _each(lambda hp, **k: hp.lift_logits(**k), lg,
                   dict({"logits D+1": ("logits", grown(d, 2)), "logits fH-1": ("logits", grown(d, 3, -1)),
                         "logits: lift_mats 4x5": ("lift_mats", grown(m, 4))},
                        **{"logits: " + k: v for k, v in _host_and_integer(lg, integer=("logits", "feat")).items()}))
    d1 = dict(depth=None, feat=f, lift_mats=m)
    cases += _each(lambda hp, **k: hp.lift(use_depth=False, **k), d1,
                   dict({"D=1: lift_mats N+1": ("lift_mats", grown(m, 1)), "D=1: feat int64": ("feat", f.long())},
                        **{"D=1: " + k: v for k, v in _host_and_integer(d1).items()}))
    ff = d.unsqueeze(2) * f.unsqueeze(3)
    dn = dict(frustum_feats=ff, lift_mats=m)
    cases += _each(lambda hp, **k: hp.lift_dense(**k), dn,
                   dict({"dense: 5-D frustum_feats": ("frustum_feats", f), "dense: lift_mats N+1": ("lift_mats", grown(m, 1)),
                         "dense: lift_mats 4x5": ("lift_mats", grown(m, 4))},
                        **{"dense: " + k: v for k, v in _host_and_integer(dn).items()}))
    for nm, fn in (("lift_indices", lambda hp, lift_mats: hp.lift_indices(lift_mats)),
                   ("lift_cull_words", lambda hp, lift_mats: hp.lift_cull_words(lift_mats))):
        cases += _each(fn, dict(lift_mats=m), {f"{nm}: 4x5": ("lift_mats", grown(m, 4)),
                                               f"{nm}: 2 rows": ("lift_mats", grown(m, 2, -1)),
                                               f"{nm}: on the host": ("lift_mats", m.cpu())})
    refusals(cfg, dev, cases)


def test_render_mistakes_raise_before_any_launch(dev):
    cfg, ins = render_scene(dev)
    vols = ("density_feature", "semantic_logits", "base", "rgb")
    wrong = {}
    for k in vols:
        for axis, nm in ((0, "B"), (2, "Z"), (3, "Y"), (4, "X")):
            wrong[f"{k} {nm}+1"] = (k, grown(ins[k], axis))
        wrong[f"{k} X-1"] = (k, grown(ins[k], 4, -1))
    for k in ("density_feature", "semantic_logits", "rgb"):
        wrong[f"{k} channels+1"] = (k, grown(ins[k], 1))
    wrong.update({"render_mats 4x5": ("render_mats", grown(ins["render_mats"], 4)),
                  "render_mats 2 rows": ("render_mats", grown(ins["render_mats"], 2, -1)),
                  "beta of two elements": ("beta", torch.zeros(2, device=dev))})
    wrong.update(_host_and_integer(ins, integer=vols))
    cases = _each(render_call, ins, wrong)
    hp0, _ = guarded(cfg, dev)
    geom = hp0.frustum_geometry(ins["render_mats"])
    gi = dict({k: v for k, v in ins.items() if k != "render_mats"}, geom=geom)
    cases += _each(render_call, gi, {"geom D+1": ("geom", grown(geom, 2)), "geom D-1": ("geom", grown(geom, 2, -1)),
                                     "geom fH+1": ("geom", grown(geom, 3)), "geom xyzw": ("geom", grown(geom, 5)),
                                     "geom on the host": ("geom", geom.cpu())})
    cases.append(("geom and render_mats", lambda hp: render_call(hp, **dict(gi, render_mats=ins["render_mats"]))))
    rm = ins["render_mats"]
    cases += _each(lambda hp, render_mats: hp.frustum_geometry(render_mats), dict(render_mats=rm),
                   {"frustum_geometry: 4x5": ("render_mats", grown(rm, 4)), "frustum_geometry: host": ("render_mats", rm.cpu())})
    cases += _each(lambda hp, render_mats: hp.render_indices(render_mats=render_mats), dict(render_mats=rm),
                   {"render_indices: 4x5": ("render_mats", grown(rm, 4)), "render_indices: host": ("render_mats", rm.cpu())})
    cases += _each(lambda hp, geom: hp.render_indices(geom=geom), dict(geom=geom),
                   {"render_indices: geom D+1": ("geom", grown(geom, 2)), "render_indices: geom host": ("geom", geom.cpu())})
    cases += _each(lambda hp, render_mats: hp.render_direct_taps(render_mats), dict(render_mats=rm),
                   {"render_direct_taps: 4x5": ("render_mats", grown(rm, 4)), "render_direct_taps: host": ("render_mats", rm.cpu())})
    st = dict(density_feature=ins["density_feature"], beta=ins["beta"], render_mats=rm)
    dens = ins["density_feature"]
    cases += _each(lambda hp, **k: hp.ert_statistics(**k), st,
                   dict({"ert_statistics: Z+1": ("density_feature", grown(dens, 2)),
                         "ert_statistics: two channels": ("density_feature", grown(dens, 1)),
                         "ert_statistics: 4x5": ("render_mats", grown(rm, 4))},
                        **{"ert_statistics: " + k: v for k, v in _host_and_integer(st, integer=("density_feature",)).items()}))
    refusals(cfg, dev, cases)


def test_resampling_and_glue_mistakes_raise_before_any_launch(dev):
    cfg, ins, pts = points_scene(dev)
    sem, dens, beta = ins["semantic_logits"], ins["density_feature"], ins["beta"]
    sp = dict(volume=dens, points=pts, beta=beta)
    call = lambda hp, **k: hp.sample_points(activation=True, **k)
    cases = _each(call, sp, dict({"volume Z+1": ("volume", grown(dens, 2)), "volume X-1": ("volume", grown(dens, 4, -1)),
                                  "points xy": ("points", grown(pts, 2, -1)), "points B+1": ("points", grown(pts, 0)),
                                  "beta of two elements": ("beta", torch.zeros(2, device=dev))},
                                 **_host_and_integer(sp, integer=("volume",))))
    cases.append(("padding", lambda hp: hp.sample_points(sem, pts, padding="reflection")))
    occ = torch.zeros(4, 3, 2, 3, device=dev)
    bda = synthetic.bda_matrix(B, rot_deg=5.0).to(dev)
    oq = dict(semantic_logits=sem, density_feature=dens, occ_coords=occ, bda_mat=bda, beta=beta)
    cases += _each(lambda hp, **k: hp.occupancy_queries(**k), oq,
                   dict({"occ: semantic Z+1": ("semantic_logits", grown(sem, 2)), "occ: density Y+1": ("density_feature", grown(dens, 3)),
                         "occ: coords xy": ("occ_coords", grown(occ, 3, -1)), "occ: bda B+1": ("bda_mat", grown(bda, 0))},
                        **{"occ: " + k: v for k, v in _host_and_integer(oq, integer=("semantic_logits", "density_feature")).items()}))
    gen = torch.Generator().manual_seed(5)
    lg = torch.randn(B * cfg.num_cams, cfg.D, cfg.fH, cfg.fW, generator=gen).to(dev)
    cases += _each(lambda hp, logits: hp.depth_softmax(logits), dict(logits=lg),
                   {"depth_softmax: host": ("logits", lg.cpu()), "depth_softmax: int64": ("logits", lg.long()),
                    "depth_softmax: 2-D": ("logits", lg[:, :, 0, 0])})
    C_, cout = 4, 8
    vo = torch.randn(B, C_, cfg.oZ, cfg.oY, cfg.oX, generator=gen).to(dev)
    vd = torch.randn(B, 1, cfg.oZ, cfg.oY, cfg.oX, generator=gen).to(dev)
    dg = dict(voxel_output=vo, voxel_density=vd)
    cases += _each(lambda hp, **k: hp.density_gate(**k), dg,
                   dict({"gate: density oZ+1": ("voxel_density", grown(vd, 2)), "gate: density 2 channels": ("voxel_density", grown(vd, 1)),
                         "gate: output oX+1": ("voxel_output", grown(vo, 4))},
                        **{"gate: " + k: v for k, v in _host_and_integer(dg, integer=("voxel_output", "voxel_density")).items()}))
    w, bs = torch.randn(cout, C_ * cfg.oZ, 1, 1, generator=gen).to(dev), torch.randn(cout, generator=gen).to(dev)
    gc = dict(voxel_output=vo, voxel_density=vd, weight=w, bias=bs)
    cases += _each(lambda hp, **k: hp.gate_conv1x1(**k), gc,
                   dict({"gate_conv: weight C*oZ+1": ("weight", grown(w, 1)), "gate_conv: bias Cout+1": ("bias", grown(bs, 0)),
                         "gate_conv: density oY+1": ("voxel_density", grown(vd, 3)), "gate_conv: output C+1": ("voxel_output", grown(vo, 1))},
                        **{"gate_conv: " + k: v for k, v in _host_and_integer(gc, integer=("voxel_output", "voxel_density", "weight")).items()}))
    refusals(cfg, dev, cases)


# ---------------------------------------------------------------------------------------------------- the module path
@pytest.mark.parametrize("hip_glue", [False, True], ids=["aten-glue", "hip-glue"])
def test_module_path_without_fusion_under_the_guard(dev, monkeypatch, hip_glue):
    """The tiny BaseVAMPIRE2 of test_backbone_forward_backward with the fused producer / consumer forms off (and the HIP
    glue kernels on), its two producing convolutions in torch.channels_last: softmax -> lift(depth, feat) with whatever
    layouts aten hands over.  No violation, and the outputs and gradients of the switch-default run at that test's
    tolerances."""
    from vampire_amd.backbone import BaseVAMPIRE2
    c = CFG_TINY
    kw = dict(x_bound_seg=list(c.x_bound_seg), y_bound_seg=list(c.y_bound_seg), z_bound_seg=list(c.z_bound_seg),
              x_bound_det=list(c.x_bound_det), y_bound_det=list(c.y_bound_det), z_bound_det=list(c.z_bound_det),
              d_bound=list(c.d_bound), final_dim=c.final_dim, downsample_factor=4, upsample_factor=4,
              mid_channels=4, output_channels=8, img_backbone_conf=dict(), img_neck_conf=dict(out_channels=[8] * 4),
              num_classes=5, density_mode="sdf", sdf_bias=-1.0, cat_pos=True, cat_seg=True)
    torch.manual_seed(0)
    ref = BaseVAMPIRE2(**kw).eval()
    with torch.no_grad():
        ref.density_conv.bias.fill_(-1.0)
    s2e, K, ida = synthetic.camera_rig(c, B, src_hw=(64, 176), focal=60.0, centre=(88.0, 34.0), jitter=2.0, seed=4)
    s2e[:, :, :3, 3] *= 0.3
    mats = dict(sensor2ego_mats=s2e[:, None], intrin_mats=K[:, None], ida_mats=ida[:, None],
                sensor2sensor_mats=torch.eye(4).expand(B, 1, 6, 4, 4), bda_mat=synthetic.bda_matrix(B, rot_deg=8.0))
    mats = {k: v.to(dev) for k, v in mats.items()}
    imgs = torch.randn(B, 1, 6, 3, *c.final_dim).to(dev)
    pts = [(torch.rand(50, 3) * 8 - 4).to(dev) for _ in range(B)]

    def step(mod, guard_it):
        guard = call_guard.install(mod.hot_path()) if guard_it else None
        x = imgs.clone().requires_grad_(True)
        out = mod(x, mats, inrange_pts=pts)
        sum((o.float() ** 2).mean() for o in out[:8]).backward()
        return out, x.grad, mod.density.beta.grad.clone(), guard

    want, want_gx, want_gb, _ = step(copy.deepcopy(ref).to(dev), False)              # the switches' defaults
    monkeypatch.setattr(backbone.SWITCHES, "fuse", False)
    monkeypatch.setattr(backbone.SWITCHES, "hip_glue", hip_glue)
    mod = copy.deepcopy(ref).to(dev)
    mod.mapping_along_depth.to(memory_format=torch.channels_last)
    mod.channel_lower.to(memory_format=torch.channels_last)
    got, got_gx, got_gb, guard = step(mod, True)
    names = [n for n, _ in guard.log]
    assert "vamp_lift_forward_ex" in names and "vamp_lift_forward_logits_ex" not in names, names
    assert ("vamp_depth_softmax_forward" in names) == hip_glue and ("vamp_density_gate_forward" in names) == hip_glue, names
    assert "vamp_gate_conv1x1_forward" not in names, names
    close(got[0], want[0], atol=2e-4, what="bev feature")
    close(got[1], want[1], what="rgb_preds")
    close(got[2], want[2], what="seg_logits_preds")
    close(got[3], want[3], atol=2e-4, what="depth_preds")
    for i in (4, 5, 6, 7):
        close(got[i], want[i], what=f"output {i}")
    for i in (8, 9):
        for a, b in zip(got[i], want[i]):
            close(a, b, atol=2e-4, what=f"output {i}")
    for i in (10, 11):
        close(got[i], want[i], atol=2e-4, what=f"output {i}")
    close(got_gx, want_gx, atol=1e-6, rtol=2e-3, scale="max", what="grad images")
    close(got_gb.reshape(1), want_gb.reshape(1), atol=1e-5, rtol=2e-3, what="grad beta")
