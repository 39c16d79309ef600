"""The four point queries of a step as one operator (vampire_amd/csrc/point_queries.hip, HotPath.point_queries): packed
lidar points with per-sample counts and the occupancy grid against the four existing calls (`sample_points` with border
/ channel_last, with mask_outside, and `occupancy_queries`) bit for bit in the forward, and against the float64 gather of
test_sample_points_sweep.py in the backward.

Shapes are the sweep's small ones (Z = 5, Y = 16, X = 5 | 33: either side of the gather's 32-voxel x-run; B = 2 | 3):
what can go wrong here is in the lists, the counts and the row widths (K + 1 = 2, 4, 19, 32: CP4 = 1, 1, 5, 8), not in
the size.  The bar of a summed gradient is the sum of the sweep's bars of its parts, each part's bar taken on that
part's own float64 reference with that part's own record counts (`part_bar`), so a voxel that only the union makes
heavy is held to the light bar.

The largest fractions of the bars seen on an MI355X are in test_gradients_against_float64's docstring."""
import ctypes as C
import dataclasses
import math

import pytest
import torch

from vampire_amd import _capi, _header
from vampire_amd.config import CFG_TINY
from test_hip_parity import close
from test_sample_points_sweep import (ACT_BETA_BAR, ACT_GRAD_BAR, BF16_GRAD_REL, GRAD_CAP, GRAD_CAP_CROWD, K_BWD_TREE,
                                      K_BWD_WEIGHT, K_PTS_HEAVY, U, Case, axes, crowd_points, ratio, reference, shared_hot,
                                      structured_points, to_ego, voxel_records)
from test_operator_contract import ROUNDING, RUN_ATOL, RUN_RTOL

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
LATTICE = (7, 5, 11)          # P = 385: one full workgroup and a ragged one


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------- inputs
def qcase(K, X=33, B=2, mode="sdf", beta=0.1):
    """The sweep's Case of the semantic volume; its cfg (bounds, density mode) is the operator's."""
    return Case(f"q-K{K}-X{X}-B{B}-{mode}{beta}", C=K, X=X, B=B, act=mode, beta=beta)


def lidar_points(case, M):
    """[B, M, 3]: the first M of the sweep's structured points of every sample (one of every kind first), repeated
    when M is larger."""
    per_b = []
    for b in range(case.B):
        rows = [r[2] for r in structured_points(case, b)]
        rows = (rows * (M // len(rows) + 1))[:M]
        per_b.append(torch.tensor(rows, dtype=F64).float().reshape(M, 3))
    return torch.stack(per_b)


def occ_grid(case):
    """An n0 x n1 x n2 lattice over the seg bounds, axis 0 along x (the layout of the Occ3D grid)."""
    lin = [torch.linspace(bnd[0], bnd[1], n, dtype=F64) for (bnd, _), n in zip(axes(case.cfg), LATTICE)]
    return torch.stack(torch.meshgrid(*lin, indexing="ij"), dim=-1).float()


def bda(B, deg=20.0, scale=1.05):
    """[B, 4, 4]: rotation about z by +-deg and a scale, so that some corners of the lattice leave the bounds."""
    m = torch.eye(4).repeat(B, 1, 1)
    for b in range(B):
        a = math.radians(deg if b % 2 == 0 else -deg)
        m[b, :2, :2] = scale * torch.tensor([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
        m[b, 2, 2] = scale
    return m


def volumes(case, seed=3):
    gen = torch.Generator().manual_seed(seed + case.C + 7 * case.X + 17 * case.B)
    shp = (case.B, 1, case.Z, case.Y, case.X)
    sem = torch.randn(case.B, case.C, *shp[2:], generator=gen)
    den = 0.5 * torch.randn(shp, generator=gen) - 1.0
    return sem, den


def beta_of(case, dev, grad=False):
    return torch.tensor(case.beta, device=dev, requires_grad=grad) if case.act == "sdf" else None


def split_calls(hp, case, sem, den, beta, pts, counts, occ_pts, sdf=True, want=(True, True, True, True)):
    """The four existing calls on the same inputs: per-sample pts_logits / pts_sdf on the rows that count, and the two
    occupancy resamplings on the points given (the rotation is the caller's, as in `occupancy_points`).  want: which
    of (pts_logits, pts_sdf, occ_logits, occ_density) to make; the others come back as an empty list or None."""
    pl, ps = [], []
    for b in range(case.B if want[0] or (want[1] and sdf) else 0):
        p = pts[b, :counts[b]][None]
        if want[0]:
            pl.append(hp.sample_points(sem[[b]], p, padding="border", channel_last=True)[0])
        if want[1] and sdf:
            ps.append(hp.sample_points(den[[b]], p, mask_outside=True)[0, 0])
    ol = hp.sample_points(sem, occ_pts, padding="border") if want[2] else None
    od = hp.sample_points(den, occ_pts, activation=True, beta=beta) if want[3] else None
    return pl, ps, ol, od


def assert_rows(got, parts, counts, what):
    """got [B, M, ...] equals the per-sample results on the rows that count and is exact 0 behind them; every element
    is compared."""
    for b, n in enumerate(counts):
        assert torch.equal(got[b, :n], parts[b]), f"{what}: sample {b}"
        assert bool((got[b, n:] == 0).all()), f"{what}: sample {b}: rows beyond the count are not 0"


# ---------------------------------------------------------------------------------------------------- 1. forward
SHAPES = [(5, 2, 1, [1, 0]), (33, 2, 63, [63, 0]), (33, 3, 257, [1, 256, 257]), (5, 2, 257, None)]
FWD = ([(K, *s, "sdf", 0.1) for K in (1, 3, 18, 31) for s in SHAPES]
       + [(3, *SHAPES[2], "sdf", 0.0), (3, *SHAPES[2], "sdf", -0.1), (18, *SHAPES[1], "sdf", -0.1),
          (3, *SHAPES[2], "naive", 0.1), (18, *SHAPES[1], "naive", 0.1)])


@gpu
@pytest.mark.parametrize("K,X,B,M,counts,mode,beta", FWD,
                         ids=[f"K{k}-X{x}-B{b}-M{m}-{'all' if c is None else 'cnt'}-{md}{bt}" for k, x, b, m, c, md, bt in FWD])
def test_forward_bit_for_bit(dev, K, X, B, M, counts, mode, beta):
    """All four outputs are torch.equal to the four existing calls on the same inputs: every point kind of the sweep
    (interior, bound, one to three voxels outside, far, 1e30, non-finite), a rotated and scaled occupancy lattice whose
    corners leave the bounds, counts of 0, 1, M - 1 and M; rows beyond a count are exact 0."""
    case = qcase(K, X, B, mode, beta)
    hp = shared_hot(case.cfg, dev)
    sem, den = (v.to(dev) for v in volumes(case))
    pts = lidar_points(case, M).to(dev)
    cnt = [M] * B if counts is None else counts
    cnt_dev = None if counts is None else torch.tensor(counts, dtype=torch.int32, device=dev)
    grid, rot = occ_grid(case).to(dev), bda(B).to(dev)
    bt = beta_of(case, dev)
    sdf = mode == "sdf"
    occ_pts = hp.occupancy_points(grid, rot)
    inside = ((occ_pts.cpu() >= torch.tensor([b[0][0] for b in axes(case.cfg)]))
              & (occ_pts.cpu() <= torch.tensor([b[0][1] for b in axes(case.cfg)]))).all(-1)
    assert bool(inside.any()) and not bool(inside.all()), "the lattice must straddle the bounds"
    q = hp.point_queries(sem, den, bt, points=pts, counts=cnt_dev, sdf=sdf, occ_points=occ_pts, lattice=LATTICE)
    pl, ps, _, _ = split_calls(hp, case, sem, den, bt, pts, cnt, occ_pts, sdf)
    ol, od = hp.occupancy_queries(sem, den, grid, rot, bt)
    assert q.pts_logits.shape == (B, M, K) and q.occ_logits.shape == (B, K, 385) and q.occ_density.shape == (B, 1, 385)
    assert_rows(q.pts_logits, pl, cnt, "pts_logits")
    if sdf:
        assert q.pts_sdf.shape == (B, M)
        assert_rows(q.pts_sdf, ps, cnt, "pts_sdf")
    else:
        assert q.pts_sdf is None
    assert torch.equal(q.occ_logits.reshape(ol.shape), ol), "occ_logits"
    assert torch.equal(q.occ_density.reshape(od.shape), od), "occ_density"
    assert all(bool(t.isfinite().all()) for t in q if t is not None)


@gpu
def test_parts_can_be_left_out(dev):
    """No lidar part, no occupancy part, no sdf, a shared [1, P, 3] grid: the parts asked for keep their bits, the
    others are None."""
    case = qcase(3, 33, 2)
    hp = shared_hot(case.cfg, dev)
    sem, den = (v.to(dev) for v in volumes(case))
    pts, grid, bt = lidar_points(case, 63).to(dev), occ_grid(case).to(dev), beta_of(case, dev)
    full = hp.point_queries(sem, den, bt, points=pts, sdf=True, occ_points=hp.occupancy_points(grid, None), lattice=LATTICE)
    ol, od = hp.occupancy_queries(sem, den, grid, None, bt)
    assert torch.equal(full.occ_logits.reshape(ol.shape), ol) and torch.equal(full.occ_density.reshape(od.shape), od)
    a = hp.point_queries(sem, None, points=pts)
    assert a.pts_sdf is None and a.occ_logits is None and a.occ_density is None and torch.equal(a.pts_logits, full.pts_logits)
    b = hp.point_queries(sem, den, bt, occ_points=hp.occupancy_points(grid, None))
    assert b.pts_logits is None and b.pts_sdf is None and torch.equal(b.occ_density, full.occ_density)
    assert torch.equal(b.occ_logits, full.occ_logits)


# ---------------------------------------------------------------------------------------------------- 2. padding
def run(hp, sem, den, beta, ups, **kw):
    """Forward + backward of one call on fresh leaves: (outputs, (grad_semantic, grad_density, grad_beta | None))."""
    s = sem.detach().clone().requires_grad_(True)
    d = None if den is None else den.detach().clone().requires_grad_(True)
    b = None if beta is None else beta.detach().clone().requires_grad_(True)
    q = hp.point_queries(s, d, b, **kw)
    outs = [(o, u) for o, u in zip(q, ups) if o is not None and u is not None]
    torch.autograd.backward([o for o, _ in outs], [u for _, u in outs])
    return q, (s.grad, None if d is None else d.grad, None if b is None else b.grad)


def two_run(a, b, what):
    for x, y, n in zip(a, b, ("grad_semantic", "grad_density", "grad_beta")):
        if x is None or y is None:
            assert x is None and y is None, n
            continue
        assert x.dtype == y.dtype and x.shape == y.shape, n
        close(x.float(), y.float(), atol=RUN_ATOL, rtol=RUN_RTOL, scale="max", what=f"{what}: {n}")


@gpu
def test_padding_is_inert(dev):
    """NaN coordinates and NaN upstream gradients in the rows beyond the counts: outputs equal the list call on the
    truncated sets, gradients agree at the two-run bar, no NaN anywhere."""
    case = qcase(18, 33, 3)
    hp = shared_hot(case.cfg, dev)
    sem, den = (v.to(dev) for v in volumes(case))
    M, counts = 257, [200, 0, 131]
    pts = lidar_points(case, M)
    finite = pts.isfinite().all(-1, keepdim=True)
    pts = torch.where(finite, pts, torch.zeros(())).to(dev)      # (this test's NaN are the padding's alone)
    occ_pts = hp.occupancy_points(occ_grid(case).to(dev), bda(3).to(dev))
    gen = torch.Generator().manual_seed(5)
    ups = [torch.randn(s, generator=gen).to(dev) for s in ((3, M, 18), (3, M), (3, 18, 385), (3, 1, 385))]
    packed, ups_nan = pts.clone(), [u.clone() for u in ups]
    for b, n in enumerate(counts):
        packed[b, n:] = float("nan")
        ups_nan[0][b, n:] = float("nan")
        ups_nan[1][b, n:] = float("nan")
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    bt = beta_of(case, dev)
    qp, gp = run(hp, sem, den, bt, ups_nan, points=packed, counts=cnt, sdf=True, occ_points=occ_pts)
    m = max(counts)
    ups_list = [ups[0][:, :m], ups[1][:, :m], ups[2], ups[3]]
    ql, gl = run(hp, sem, den, bt, ups_list, points=[pts[b, :n] for b, n in enumerate(counts)], sdf=True, occ_points=occ_pts)
    assert ql.pts_logits.shape == (3, m, 18)
    assert torch.equal(qp.pts_logits[:, :m], ql.pts_logits) and torch.equal(qp.pts_sdf[:, :m], ql.pts_sdf)
    assert bool((qp.pts_logits[:, m:] == 0).all()) and bool((qp.pts_sdf[:, m:] == 0).all())
    assert torch.equal(qp.occ_logits, ql.occ_logits) and torch.equal(qp.occ_density, ql.occ_density)
    for t in list(qp) + list(gp):
        assert bool(t.isfinite().all())
    two_run(gp, gl, "packed vs list")


# ---------------------------------------------------------------------------------------------------- 3. gradients
def part_bar(ref, act):
    """The sweep's bar of one call's grad_volume, per element (test_sample_points_sweep.errors), on that call's own
    float64 reference and record counts."""
    gmax = float(ref.gvol.abs().max())
    if act:
        return torch.full_like(ref.gvol, ACT_GRAD_BAR * (1 + gmax))
    n = ref.nrec[:, None].double()
    cap = torch.where(n > K_PTS_HEAVY, torch.full_like(n, GRAD_CAP_CROWD), torch.full_like(n, GRAD_CAP)) * gmax
    return torch.minimum((K_BWD_WEIGHT + n + K_BWD_TREE) * U * ref.A_g, cap.expand_as(ref.A_g))


def crowded_scene(case, sites=((4, 2, 2), (20, 9, 2))):
    """B = 3.  Sample 0: a voxel with 200 lidar + 100 occupancy records (heavy through the union alone) and one with
    600 lidar records; sample 1: plain sets; sample 2: count 0.  Returns (pts [3, M, 3], counts, occ [3, P, 3], sites)."""
    s_union, s_big = sites
    border = dataclasses.replace(case, padding="border")
    lid = [lidar_points(case, 150)[b] for b in range(3)]
    lid = [torch.where(p.isfinite().all(-1, keepdim=True), p, torch.zeros(())) for p in lid]
    lid[0] = torch.cat([lid[0], crowd_points(border, 0, lid[0], s_union, 200)])
    lid[0] = torch.cat([lid[0], crowd_points(border, 0, lid[0], s_big, 600)])
    counts = [len(lid[0]), len(lid[1]), 0]
    M = counts[0]
    pts = torch.full((3, M, 3), float("nan"))
    for b in (0, 1):
        pts[b, :counts[b]] = lid[b]
    rot = torch.matmul(occ_grid(case).reshape(1, -1, 3), bda(3)[:, :3, :3].transpose(1, 2))
    zeros = dataclasses.replace(case, padding="zeros")
    extra = crowd_points(zeros, 0, rot[0], s_union, 100)
    fill = torch.stack([to_ego(torch.full((len(extra),), 0.5 + a, dtype=F64), bnd, n).float()
                        for a, (bnd, n) in enumerate(axes(case.cfg))], dim=-1)
    occ = torch.stack([torch.cat([rot[0], extra]), torch.cat([rot[1], fill]), torch.cat([rot[2], fill])])
    return pts, counts, occ, (s_union, s_big)


def gradient_check(dev, case, scene, *, f64=True, lidar=True, occupancy=True, sdf=True, shared=False,
                   given=(True, True, True, True), den_dtype=F32, tag=None):
    """One fused backward on `scene` (crowded_scene's tuple) against the float64 gather summed over the queries asked
    for, and against the sum of the existing backward calls of the same queries, both at the sum of the parts' bars
    (part_bar; grad_beta at ACT_BETA_BAR of the sum of its terms' magnitudes).  lidar / occupancy: the point sets given;
    sdf: pts_sdf asked for; shared: one [1, P, 3] grid (sample 0's) for every sample; given: which of the four outputs
    get an upstream gradient (the others add nothing, in the references as well); den_dtype bfloat16: the density
    volume's values are bf16 values and grad_density comes back rounded once to bf16, which the comparison allows for
    as the sweep's `errors` does.  With f64 false the float64 figures are printed and not held (beta = 0).  Prints every
    fraction of its bar and returns {(reference, gradient): fraction}."""
    K = case.C
    tag = tag or f"K{K} beta{case.beta}"
    hp = shared_hot(case.cfg, dev)
    sem, den = volumes(case)
    if den_dtype != F32:
        den = den.to(den_dtype).float()
    pts, counts, occ, (s_union, s_big) = scene
    B = case.B
    if shared:
        occ = occ[:1]
    occ_b = occ.expand(B, -1, -1)
    M, P = pts.shape[1], occ.shape[1]
    gen = torch.Generator().manual_seed(11 + K)
    ups = [torch.randn(s, generator=gen) for s in ((B, M, K), (B, M), (B, K, P), (B, 1, P))]
    has = (lidar, lidar and sdf, occupancy, occupancy)
    ups = [u if g else torch.zeros_like(u) for u, g in zip(ups, given)]          # (the references' upstream: zeros)
    ups_dev = [u.to(dev) if h and g else None for u, h, g in zip(ups, has, given)]
    assert any(u is not None for u in ups_dev)
    # the float64 parts: rows beyond a count carry no gradient and sit at a harmless interior point
    live = torch.arange(M)[None] < torch.tensor(counts)[:, None]
    centre = torch.tensor([to_ego(1.5 if n > 2 else 0.5, bnd, n) for bnd, n in axes(case.cfg)], dtype=F32)
    p_ref = torch.where(live[..., None], pts, centre)
    u0 = torch.where(live[..., None], ups[0], torch.zeros(())).permute(0, 2, 1)
    u1 = torch.where(live, ups[1], torch.zeros(()))[:, None]
    c_sem = dataclasses.replace(case, padding="border", act="")
    c_sdf = dataclasses.replace(case, C=1, mask=True, act="")
    c_den = dataclasses.replace(case, C=1)
    refs = {}
    if has[0]:
        refs["pl"] = reference(c_sem, sem, p_ref, u0)
    if has[1]:
        refs["ps"] = reference(c_sdf, den, p_ref, u1)
    if has[2]:
        refs["ol"], refs["od"] = reference(c_sem, sem, occ_b, ups[2]), reference(c_den, den, occ_b, ups[3])
    # record counts of the lidar parts: the rows that count alone (the bars take them from here)
    for key, c_part in (("pl", c_sem), ("ps", c_sdf)):
        if key in refs:
            refs[key].nrec = torch.cat([voxel_records(case.cfg, pts[b:b + 1, :n], c_part.border, c_part.mask)
                                        for b, n in enumerate(counts)])
    # the crowds are there
    zero_n = torch.zeros(B, case.Z, case.Y, case.X, dtype=torch.int64)
    n_l = refs["pl"].nrec if lidar else zero_n
    n_o = voxel_records(case.cfg, occ_b, True, False) if occupancy else zero_n
    at = lambda n, s: int(n[0, s[2], s[1], s[0]])
    if lidar:
        assert at(n_l, s_union) == 200 and at(n_l, s_big) >= 600, (at(n_l, s_union), at(n_l, s_big))
    if occupancy:
        assert at(n_o, s_union) == 100, at(n_o, s_union)
    zero_v = torch.zeros(B, 1, case.Z, case.Y, case.X, dtype=F64)
    parts = lambda keys, acts: (sum((refs[k].gvol for k in keys if k in refs), zero_v),
                                sum((part_bar(refs[k], a) for k, a in zip(keys, acts) if k in refs), zero_v))
    ref_sem, bar_sem = parts(("pl", "ol"), (False, False))
    ref_den, bar_den = parts(("ps", "od"), (False, True))
    want_den = has[1] or occupancy
    want_beta = occupancy and case.act == "sdf"
    bar_beta = ACT_BETA_BAR * max(refs["od"].gscale, 1e-300) if want_beta else None

    to = lambda t: t.to(dev)
    cnt = torch.tensor(counts, dtype=torch.int32, device=dev)
    bt = beta_of(case, dev) if occupancy else None
    den_dev = to(den).to(den_dtype) if want_den else None
    kw = {}
    if lidar:
        kw.update(points=to(pts), counts=cnt, sdf=sdf)
    if occupancy:
        kw.update(occ_points=to(occ))
    _, got = run(hp, to(sem), den_dev, bt, ups_dev, **kw)
    assert (got[1] is not None) == want_den and (got[2] is not None) == want_beta
    assert got[1] is None or got[1].dtype == den_dtype
    # the existing backward calls of the same queries, summed
    s = to(sem).requires_grad_(True)
    # (a 16-bit density leaf would get each call's gradient rounded to 16 bits and their sum rounded again: the calls
    # run on the same values in fp32, as in test_dtype_mixes, and the fused gradient's one rounding is allowed for below)
    d = den_dev.float().clone().requires_grad_(True) if want_den else None
    b = bt.clone().requires_grad_(True) if bt is not None else None
    want = [u is not None for u in ups_dev]
    pl, ps, ol, od = split_calls(hp, case, s, d, b, to(pts), counts, to(occ_b).contiguous(), sdf, want)
    outs = pl + ps + [o for o in (ol, od) if o is not None]
    gr = ([ups_dev[k][i, :n] for k, part in ((0, pl), (1, ps)) if part for i, n in enumerate(counts)]
          + [ups_dev[k] for k, o in ((2, ol), (3, od)) if o is not None])
    torch.autograd.backward(outs, gr)
    grad64 = lambda t, like: torch.zeros_like(like) if t is None or t.grad is None else t.grad.cpu().double()
    calls = (grad64(s, ref_sem), grad64(d, ref_den), float(b.grad) if want_beta and b.grad is not None else 0.0)
    seen, bad = {}, []
    for name, ref_g in (("float64", (ref_sem, ref_den, refs["od"].gbeta if want_beta else None)), ("four calls", calls)):
        figures = [("grad_semantic", ratio((got[0].cpu().double() - ref_g[0]).abs(), bar_sem))]
        if want_den:
            d_den = (got[1].cpu().double() - ref_g[1]).abs()
            if den_dtype == torch.bfloat16:           # the fp32 gradient rounded once to bf16's 8-bit significand
                d_den = (d_den - BF16_GRAD_REL * ref_g[1].abs()).clamp_min(0)
            figures.append(("grad_density", ratio(d_den, bar_den)))
        if want_beta:
            figures.append(("grad_beta", abs(float(got[2]) - ref_g[2]) / bar_beta))
        for what, e in figures:
            print(f"SEEN {tag} vs {name} {what}: {e:.3e} of the bar")
            seen[(name, what)] = e
            if not e <= 1.0 and (f64 or name != "float64"):
                bad.append(f"{name} {what}: {e:.3e} of the bar")
    assert not bad, "\n".join(bad)
    return seen, n_l, n_o


@gpu
@pytest.mark.parametrize("K,beta,f64", [(18, 0.1, True), (3, -0.1, True), (31, 0.0, False)],
                         ids=["K18-beta0.1", "K3-beta-0.1", "K31-beta0-four-calls"])
def test_gradients_against_float64(dev, K, beta, f64):
    """grad_semantic, grad_density and grad_beta of one backward against the float64 gather summed over the four
    queries, and against the sum of the four existing backward calls, both at the sum of the parts' bars.

    Largest fraction of the bar seen on an MI355X: against float64 grad_semantic 0.23, grad_density 0.063, grad_beta
    0.25; against the four calls grad_semantic 0.23, grad_density 0.051, grad_beta 0.13.

    beta = 0 (beta_eff = beta_min = 1e-4) is held to the four existing calls only.  There d sigma / d s = -0.5 e / beta^2
    with e = expm1(-|t| / beta) + 1 (density_all): the sum rounds at 6e-8 absolute, so the derivative carries an
    absolute error of 3 per unit of upstream gradient whatever e is, while ACT_GRAD_BAR is relative to the largest
    gradient, which is set by the smallest |t| among the voxels the points touch -- a property of the random volume,
    not of the kernel.  On this file's volume the fused backward is 3.24 of that bar away from float64 and 2e-6 of it
    away from the four existing calls, which are as far from float64 as it is: the figure is the activation's, which
    this operator shares with `sample_points` unchanged."""
    case = qcase(K, 33, 3, "sdf", beta)
    _, n_l, n_o = gradient_check(dev, case, crowded_scene(case), f64=f64)
    assert int(n_l[2].sum()) == 0 and int(n_o[2].sum()) > 0            # sample 2: no lidar point, its grid alone


# ---------------------------------------------------------------------------------------------------- 4. dtypes
def small_scene(case, dev, M=63, counts=(63, 17)):
    sem, den = (v.to(dev) for v in volumes(case))
    pts = lidar_points(case, M).to(dev)
    hp = shared_hot(case.cfg, dev)
    occ_pts = hp.occupancy_points(occ_grid(case).to(dev), bda(case.B).to(dev))
    gen = torch.Generator().manual_seed(23)
    K, P = case.C, occ_pts.shape[1]
    ups = [torch.randn(s, generator=gen).to(dev) for s in ((case.B, M, K), (case.B, M), (case.B, K, P), (case.B, 1, P))]
    kw = dict(points=pts, counts=torch.tensor(counts, dtype=torch.int32, device=dev), sdf=True, occ_points=occ_pts,
              lattice=LATTICE)
    return hp, sem, den, beta_of(case, dev), ups, kw


@gpu
@pytest.mark.parametrize("sem_dt,den_dt", [(torch.bfloat16, F32), (F32, torch.bfloat16), (torch.float16, F64)],
                         ids=["bf16-sem", "bf16-den", "fp16-fp64"])
def test_dtype_mixes(dev, sem_dt, den_dt):
    """16-bit semantic with fp32 density and the reverse against the same values in fp32: equal outputs, each
    gradient in its volume's dtype within that dtype's one rounding; fp16 and fp64 volumes are promoted."""
    hp, sem, den, bt, ups, kw = small_scene(qcase(18, 33, 2), dev)
    sem_t, den_t = sem.to(sem_dt), den.to(den_dt)
    q, g = run(hp, sem_t, den_t, bt, ups, **kw)
    q32, g32 = run(hp, sem_t.float(), den_t.float(), bt, ups, **kw)
    for a, b_ in zip(q, q32):
        assert a.dtype == F32 and torch.equal(a, b_)
    assert g[0].dtype == sem_dt and g[1].dtype == den_dt
    for got, ref, dt, n in ((g[0], g32[0], sem_dt, "grad_semantic"), (g[1], g32[1], den_dt, "grad_density")):
        err = (got.double() - ref.double()).abs() - ROUNDING[dt] * ref.double().abs()
        assert float(err.max()) <= RUN_ATOL + RUN_RTOL * float(ref.abs().max()), n
    close(g[2], g32[2], atol=RUN_ATOL, rtol=RUN_RTOL, scale="max", what="grad_beta")


# ---------------------------------------------------------------------------------------------------- 5. layouts, refusals
def _strided(t):
    big = torch.zeros(tuple(2 * s for s in t.shape), dtype=t.dtype, device=t.device)
    v = big[tuple(slice(None, None, 2) for _ in t.shape)]
    v.copy_(t)
    return v


def _permuted(t):
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def _odd_offset(t):
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


@gpu
@pytest.mark.parametrize("view", [_strided, _permuted, _odd_offset], ids=["strided", "permuted", "odd-offset"])
def test_layouts_give_the_same_bits(dev, view):
    hp, sem, den, bt, ups, kw = small_scene(qcase(3, 33, 2), dev)
    q, g = run(hp, sem, den, bt, ups, **kw)
    kv = dict(kw, points=view(kw["points"]), occ_points=view(kw["occ_points"]), counts=_strided(kw["counts"]))
    sv, dv = view(sem), view(den)
    assert view is _odd_offset or not sv.is_contiguous()
    qv, gv = run(hp, sv, dv, bt, [view(u) for u in ups], **kv)
    for a, b_ in zip(q, qv):
        assert torch.equal(a, b_)
    two_run(gv, g, "layout")


@gpu
def test_refusals_raise_before_a_launch(dev):
    """Host tensors, wrong shapes, integer volumes, counts with a list, sdf without a density volume and K = 32 raise
    before any library call (the library object is replaced by one that fails the test when it is touched)."""
    case = qcase(3, 33, 2)
    hp, sem, den, bt, ups, kw = small_scene(case, dev)
    pts, occ_pts, cnt = kw["points"], kw["occ_points"], kw["counts"]

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was reached")

    real, hp.vamp = hp.vamp, Untouchable()
    try:
        err = (_capi.VampireHipError, ValueError, TypeError)
        bad = [dict(s=sem.cpu()), dict(d=den.cpu()), dict(points=pts.cpu()), dict(occ_points=occ_pts.cpu()),
               dict(counts=cnt.cpu()), dict(b=bt.cpu()),
               dict(s=sem[:, :, :-1]), dict(d=den[:, :, :, :-1]), dict(d=sem), dict(points=pts[:1]),
               dict(points=pts[..., :2]), dict(occ_points=occ_pts[..., :2]), dict(counts=cnt.long()),
               dict(counts=cnt[:1]), dict(lattice=(7, 5, 10)), dict(b=torch.zeros(2, device=dev)),
               dict(s=sem.long()), dict(d=den.int()),
               dict(points=[pts[0], pts[1]], counts=cnt), dict(points=[pts[0]]), dict(d=None), dict(d=None, sdf=False),
               dict(s=torch.zeros(2, 32, *sem.shape[2:], device=dev)), dict(b=None)]
        for change in bad:
            k = dict(kw, **{n: v for n, v in change.items() if n not in ("s", "d", "b")})
            with pytest.raises(err):
                hp.point_queries(change.get("s", sem), change.get("d", den), change.get("b", bt), **k)
    finally:
        hp.vamp = real
    assert hp.point_queries(torch.zeros(2, 31, *sem.shape[2:], device=dev), den, bt, **kw).pts_logits.shape == (2, 63, 31)


# ---------------------------------------------------------------------------------------------------- 6. sync, replay
@gpu
def test_no_sync_and_graph_replay(dev):
    """The list and the packed call forward + backward under the sync debug mode; then the operator alone, forward +
    backward, in a graph whose points, counts, volumes and upstream gradients are overwritten in place before each of
    three replays with other counts (0 and M among them): outputs equal the eager call's, gradients within the
    two-run bar."""
    case = qcase(18, 33, 3)
    hp = shared_hot(case.cfg, dev)
    M = 257
    sem, den = (v.to(dev) for v in volumes(case))
    pts = lidar_points(case, M)
    pts = torch.where(pts.isfinite().all(-1, keepdim=True), pts, torch.zeros(())).to(dev)
    occ_pts = hp.occupancy_points(occ_grid(case).to(dev), bda(3).to(dev)).contiguous()
    counts = torch.tensor([M, 100, 3], dtype=torch.int32, device=dev)
    bt = beta_of(case, dev)
    gen = torch.Generator().manual_seed(41)
    ups = [torch.randn(s, generator=gen).to(dev) for s in ((3, M, 18), (3, M), (3, 18, 385), (3, 1, 385))]
    kw = dict(points=pts, counts=counts, sdf=True, occ_points=occ_pts, lattice=LATTICE)
    def step():
        q = hp.point_queries(s_in, d_in, b_in, **kw)
        return q, torch.autograd.grad(list(q), [s_in, d_in, b_in], ups)

    lists = [pts[0].clone(), pts[1, :100].clone(), pts[2, :3].clone()]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ql, gl = run(hp, sem, den, bt, ups, points=lists, sdf=True, occ_points=occ_pts, lattice=LATTICE)
        q0, g0 = run(hp, sem, den, bt, ups, **kw)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            # the captured leaves first meet autograd on the capture stream and no backward has run on them anywhere
            # else: their gradient accumulators belong to it and the captured backward stays on the one stream (an
            # eager backward on the default stream before the capture ends the process inside capture_end)
            s_in, d_in, b_in = (t.clone().requires_grad_(True) for t in (sem, den, bt))
            step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            qg, gg = step()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    for a, b_ in zip(ql, q0):
        assert torch.equal(a, b_)
    two_run(gl, g0, "list vs packed")
    for seed, new_counts in ((1, [0, M, 77]), (2, [M, M, M]), (3, [5, 0, 0])):
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            s_in.copy_(torch.randn(sem.shape, generator=gen).to(dev))
            d_in.copy_((0.5 * torch.randn(den.shape, generator=gen) - 1.0).to(dev))
            pts.copy_((pts.cpu() + 0.3 * torch.randn(pts.shape, generator=gen)).to(dev))
            occ_pts.copy_((occ_pts.cpu() + 0.2 * torch.randn(occ_pts.shape, generator=gen)).to(dev))
            for u in ups:
                u.copy_(torch.randn(u.shape, generator=gen).to(dev))
            counts.copy_(torch.tensor(new_counts, dtype=torch.int32).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        got_q, got_g = [t.clone() for t in qg], [t.clone() for t in gg]
        q1, g1 = step()
        for a, b_ in zip(got_q, q1):
            assert torch.equal(a, b_), (seed,)
        two_run(got_g, g1, f"replay {seed}")
        for b_, n in enumerate(new_counts):
            assert bool((got_q[0][b_, n:] == 0).all()) and (n == 0 or bool((got_q[0][b_, :n] != 0).any()))


# ---------------------------------------------------------------------------------------------------- 7. module
def _module(name, mode, dev):
    import vampire_amd.backbone as BB
    c = CFG_TINY
    kw = dict(x_bound_seg=list(c.x_bound_seg), y_bound_seg=list(c.y_bound_seg), z_bound_seg=list(c.z_bound_seg),
              x_bound_det=list(c.x_bound_det), y_bound_det=list(c.y_bound_det), z_bound_det=list(c.z_bound_det),
              d_bound=list(c.d_bound), final_dim=c.final_dim, downsample_factor=4, upsample_factor=4,
              mid_channels=4, output_channels=8, img_backbone_conf=dict(), img_neck_conf=dict(out_channels=[8] * 4),
              num_classes=5, density_mode=mode, sdf_bias=-1.0)
    if name == "BaseVAMPIRE2":
        kw.update(cat_pos=True, cat_seg=False)
    torch.manual_seed(0)
    mod = getattr(BB, name)(**kw).to(dev)
    with torch.no_grad():
        mod.density_conv.bias.fill_(-1.0)
    return mod


@gpu
@pytest.mark.parametrize("name,mode", [("BaseVAMPIRE2", "sdf"), ("BaseVAMPIRE2", "naive"), ("BaseLSSImpaintor", "sdf")])
def test_module_fused_against_split(dev, monkeypatch, name, mode):
    """The module at the tiny configuration, batch 2 with unequal point counts: the 12 outputs of VAMP_QUERIES=fused
    are torch.equal to split's, parameter gradients within the two-run bar."""
    import vampire_amd.backbone as BB
    from vampire_amd import synthetic
    c, B = CFG_TINY, 2
    mod = _module(name, mode, dev)
    s2e, K, ida = synthetic.camera_rig(c, B, src_hw=(64, 176), focal=60.0, centre=(88.0, 34.0), jitter=2.0, seed=4)
    s2e[:, :, :3, 3] *= 0.3
    mats = dict(sensor2ego_mats=s2e[:, None], intrin_mats=K[:, None], ida_mats=ida[:, None],
                sensor2sensor_mats=torch.eye(4).expand(B, 1, 6, 4, 4), bda_mat=synthetic.bda_matrix(B, rot_deg=8.0))
    mats = {k: v.to(dev) for k, v in mats.items()}
    gen = torch.Generator().manual_seed(2)
    imgs = torch.randn(B, 1, 6, 3, *c.final_dim, generator=gen).to(dev)
    pts = [(torch.rand(n, 3, generator=gen) * 14 - 7).to(dev) for n in (50, 23)]

    def once(kind):
        monkeypatch.setattr(BB.SWITCHES, "queries", kind)
        mod.zero_grad(set_to_none=True)
        out = mod(imgs, mats, inrange_pts=pts)
        flat = [t for o in out for t in (o if isinstance(o, list) else [o]) if t is not None]
        sum((t.float() ** 2).mean() for t in flat).backward()
        return out, {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}

    split, g_split = once("split")
    fused, g_fused = once("fused")
    assert len(split) == len(fused) == 12
    for i, (a, b_) in enumerate(zip(split, fused)):
        if isinstance(a, list):
            assert len(a) == len(b_) == (0 if (i == 9 and mode != "sdf") else B), i
            for x, y in zip(a, b_):
                assert x.shape == y.shape and torch.equal(x, y), i
        else:
            assert a.shape == b_.shape and torch.equal(a, b_), i
    assert [t.shape[0] for t in fused[8]] == [50, 23]
    assert set(g_split) == set(g_fused) and len(g_split) > 10
    for n in g_split:
        close(g_fused[n], g_split[n], atol=RUN_ATOL, rtol=RUN_RTOL, scale="max", what=n)


# ---------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    from vampire_amd.build import build_library
    build_library(verbose=False)
    return _capi.load()


def query_desc(K=18, X=33, Y=16, Z=5, B=2, M=63, P=385):
    from vampire_amd.queries import query_desc as make
    cfg = qcase(K if 0 < K < 32 else 3, X if X > 0 else 33).cfg
    d = make(cfg, B, K, _capi.VAMP_F32, _capi.VAMP_F32, M, True, P, False, LATTICE)
    d.X, d.Y, d.Z = X, Y, Z
    return d


def test_descriptor_size_matches_the_header():
    fields = _header.read().structs["VampQueryDesc"]
    words = 0
    for name, ctype, dims in fields:
        assert ctype in ("int32_t", "float"), (name, ctype)
        words += math.prod(dims)
    assert words == 23 and C.sizeof(_capi.VampQueryDesc) == 4 * words
    assert [f[0] for f in _capi.VampQueryDesc._fields_] == [name for name, _, _ in fields]


def test_refusals_need_no_pointer(lib):
    """Bad K, extents, dtypes and a negative M are refused by the descriptor alone (every pointer is NULL), forward
    and backward; `supported` says 0 and `workspace_bytes` 0 for each; the valid descriptor gets to the pointer check."""
    nul = [None] * 11
    ok = query_desc()
    assert lib.vamp_point_queries_supported(C.byref(ok)) == 1 and lib.vamp_point_queries_workspace_bytes(C.byref(ok)) > 0
    assert lib.vamp_point_queries_forward(C.byref(ok), *nul) == -1 and b"null pointer" in lib.vamp_last_error()
    assert lib.vamp_point_queries_backward(C.byref(ok), *([None] * 13), 0, None) == -1
    assert b"null pointer" in lib.vamp_last_error()
    bad = [(query_desc(K=0), b"K + 1 <= 32"), (query_desc(K=32), b"K + 1 <= 32"), (query_desc(X=0), b"volume extents"),
           (query_desc(X=2047), b"volume extents"), (query_desc(Z=511), b"volume extents"), (query_desc(M=-1), b"M >= 0"),
           (query_desc(P=-1), b"M >= 0")]
    for field, msg in (("sem_dtype", b"sem_dtype"), ("den_dtype", b"den_dtype")):
        d = query_desc()
        setattr(d, field, _capi.VAMP_F16)
        bad.append((d, msg))
    d = query_desc()
    d.span[1] = 0.0
    bad.append((d, b"zero span"))
    for d, msg in bad:
        assert lib.vamp_point_queries_supported(C.byref(d)) == 0
        assert lib.vamp_point_queries_workspace_bytes(C.byref(d)) == 0
        assert lib.vamp_point_queries_forward(C.byref(d), *nul) == -1 and msg in lib.vamp_last_error(), msg
        assert lib.vamp_point_queries_backward(C.byref(d), *([None] * 13), 0, None) == -1
        assert msg in lib.vamp_last_error(), msg
    assert lib.vamp_point_queries_supported(None) == 0 and lib.vamp_point_queries_workspace_bytes(None) == 0


def test_python_mirror_of_supported(lib):
    from vampire_amd.queries import point_queries_supported
    for K in range(1, 41):
        for X, M, P in ((33, 63, 385), (2046, 0, 0), (2047, 63, 0), (33, -1, 0), (33, 2 ** 30, 2 ** 29)):
            d = query_desc(K=K, X=X, M=M, P=P)
            assert bool(lib.vamp_point_queries_supported(C.byref(d))) == point_queries_supported(2, K, 5, 16, X, M, P), (K, X, M, P)
    assert not point_queries_supported(2, 32, 5, 16, 33) and point_queries_supported(2, 31, 5, 16, 33)


def test_padding_helper_is_what_pack_points_did():
    """`_tensors._pad_samples` against the expressions it was moved from (labels._pack_points at the parent commit)."""
    from vampire_amd._tensors import _pad_samples
    gen = torch.Generator().manual_seed(0)
    points = [torch.randn(n, 4, generator=gen) for n in (5, 0, 9)]
    labels = [torch.randint(0, 17, (n,), generator=gen) for n in (5, 0, 9)]
    pad = torch.nn.utils.rnn.pad_sequence
    want = (pad(list(points), batch_first=True), pad(list(labels), batch_first=True),
            torch.stack([torch.full((), p.shape[0], dtype=torch.int32) for p in points]))
    got = _pad_samples(points, labels)
    assert len(got) == 3
    for a, b_ in zip(got, want):
        assert a.dtype == b_.dtype and torch.equal(a, b_)
    p_only, counts = _pad_samples(points)
    assert torch.equal(p_only, want[0]) and torch.equal(counts, want[2]) and p_only.shape == (3, 9, 4)
