"""Point resampling (vampire_amd/csrc/sample_points.hip: occ_logits, occ_density, pts_logits, pts_sdf) across the values
that pick its compiled bodies and paths -- C (the backward's eight widths CP4 = 1 ... 8, each full and with three pad
channels), the extents either side of the gather's 32-voxel x-run and down to size-1 axes, B, P, padding x mask_outside
x channel_last, the density activation with grad_beta of either sign, bf16 volumes, the lattice hint, a reused workspace
-- against a plain float64 gather written out below (not grid_sample): every output and every gradient.

One axis moves at a time from the base case (B = 2, C = 5, a 5 x 16 x 16 volume, zeros padding, fp32; CFG_TINY's seg
grid).  The point set of a case is built from classes of positions (POINT_KINDS): interior, voxel centres, the bounds,
0.3 and 0.9 of a voxel outside on one, two and all three axes -- among them the cell of floors (-1, -1, -1), whose
packed key is 0 -- further outside, +-1e3, +-1e30, NaN / +-inf, and three crowds whose record counts at one voxel are
exactly kPtsHeavy = 256 (the light gather's last), 257 at voxel (0, 0, 0) (the heavy kernel's first; in zeros padding
partly out of the low-corner cell) and 600.  The CPU tests at the end pin the gather to aten in float64, and assert from
the reference's own floors and per-cell counts that every class is there in every case: coverage is a property of the
inputs, checked without a GPU.

GPU time: shapes are at most 5 x 16 x 70 voxels and 3 x 1500 points; the file's 52 GPU tests take 3.4 s on an MI355X
(the base case 1.0 s, with the first HotPath; the others under 0.15 s each, most of it the float64 reference on the
host), its 65 CPU tests 6 s."""
import ctypes as C
import dataclasses
import functools
import itertools
import types

import numpy as np
import pytest
import torch

from oracle import aten_oracle as O
from vampire_amd import _capi
from vampire_amd.config import CFG_TINY
from test_hip_parity import hot
from test_bev_grid_sweep import bound
from test_render_shape_sweep import BF16_GRAD_REL

F64 = torch.float64
F32 = torch.float32
TINY = CFG_TINY
U = 2.0 ** -24                # one fp32 rounding, relative

# ---------------------------------------------------------------------------------------------------- the constants
K_PTS_HEAVY = 256             # kPtsHeavy: a voxel with more records goes to sample_points_heavy_kernel
PVPB = 32                     # voxels of one x-run per gather workgroup (256 / PGL)
MAX_C = 32

# ---------------------------------------------------------------------------------------------------- the bars
# Without the activation the bars are derived per element: K roundings of 2^-24 each, relative to A = sum |w v| -- the
# same reference evaluated on |volume| (forward) or |grad_out| (backward); the weights are not negative.  The fp32 tap
# coordinates are the reference's own bits and w0 = floor + 1 - f, w1 = f - floor are exact in fp32, so nothing else
# rounds.
K_FWD = 3 + 8                 # three weight products, eight fma                                 (0.43 of the bar seen)
K_BWD_WEIGHT = 3              # backward, per record: the three factors of its weight ...
K_BWD_TREE = 8                # ... the reduction: 6 halving steps and 2 adds over four waves (heavy; light: 3 steps)
#                               ... and n fma for the n records of the voxel (the longest chain one lane could have)
#                                                                                                (0.24 of the bar seen)
# ... and never looser than what this kernel's tests in test_hip_parity.py allow:
OUT_ATOL, OUT_RTOL = 1e-5, 1e-5           # outputs: 1e-5 + 1e-5 |ref|
GRAD_CAP = 2e-5                           # gradients: of max |ref|
GRAD_CAP_CROWD = 1e-4                     # ... at a voxel with more than kPtsHeavy records
# With the activation the device's expm1 / exp add ulps that are not derived here: test_point_resampling_tiny's bars
# (1e-5 + 1e-5 |ref|; gradients 1e-5 + 1e-5 max |ref|; grad_beta 1e-3), tightened to at most ten times the largest
# error seen over the sweep.
ACT_OUT_BAR = 3e-6            # max |out - ref| / (1 + |ref|)                                    3.5e-7 seen (sdf0)
ACT_GRAD_BAR = 2e-6           # max |grad - ref| / (1 + max |ref|)                               2.3e-7 seen (sdf+0.1)
ACT_BETA_BAR = 2e-7           # |grad_beta - ref| / the sum of its terms' magnitudes             2.7e-8 seen (sdf+0.1)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    C: int = 5
    X: int = 16
    Y: int = 16
    Z: int = 5
    B: int = 2
    P: int = 0                # 0: the whole point set with its crowds; P > 0: the first P points of its order, no crowds
    padding: str = "zeros"
    mask: bool = False
    channel_last: bool = False
    act: str = ""             # "", "sdf" or "naive": the density activation on the taps (C = 1)
    beta: float = 0.1
    bf16: bool = False

    @property
    def cfg(self):
        return dataclasses.replace(TINY, x_bound_seg=bound(-6.4, self.X, 0.8), y_bound_seg=bound(-6.4, self.Y, 0.8),
                                   z_bound_seg=bound(-2.0, self.Z, 0.8), density_mode=self.act or "sdf")

    @property
    def border(self):
        return self.padding == "border"


CHANNELS = [1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32]      # CP4 = 1 ... 8: full, and three pad channels
EXTENT_X = [1, 5, 31, 32, 33, 70]
POINTS = [1, 63, 65, 256, 257]
BASE = Case("base")
CASES = ([BASE]
         + [Case(f"C{c}", C=c) for c in CHANNELS if c != 5]
         + [Case(f"X{x}", X=x, Y=16, Z=5) for x in EXTENT_X]
         + [Case("Y1", Y=1), Case("Z1", Z=1)]
         + [Case(f"B{b}", B=b) for b in (1, 3)]
         + [Case(f"P{p}", P=p) for p in POINTS]
         + [Case(f"{pad}{'-mask' if m else ''}{'-chlast' if cl else ''}", padding=pad, mask=m, channel_last=cl)
            for pad in ("zeros", "border") for m in (False, True) for cl in (False, True) if (pad, m, cl) != ("zeros", False, False)]
         + [Case("sdf+0.1", C=1, act="sdf", beta=0.1), Case("sdf-0.1", C=1, act="sdf", beta=-0.1),
            Case("sdf0", C=1, act="sdf", beta=0.0), Case("naive", C=1, act="naive"),
            Case("sdf-border-mask", C=1, act="sdf", padding="border", mask=True)]
         + [Case(f"bf16-C{c}", C=c, bf16=True) for c in (1, 5, 18)]
         + [Case("bf16-sdf", C=1, act="sdf", bf16=True), Case("X33-border-C18", X=33, C=18, padding="border"),
            Case("X70-mask-C9", X=70, C=9, mask=True)])
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------- the reference
def axes(cfg):
    return ((cfg.x_bound_seg, cfg.vX), (cfg.y_bound_seg, cfg.vY), (cfg.z_bound_seg, cfg.vZ))


def axis_tap(p, bnd, n, border=False):
    """point_tap's arithmetic on one axis, operation by operation in fp32 (the library is built without contraction and
    with IEEE division, so these are its bits): the normalised coordinate g and the tap coordinate f.  Border padding:
    fminf(n - 1, fmaxf(f, 0)), which turns a NaN into 0."""
    assert p.dtype == F32
    lo = torch.tensor(bnd[0], dtype=F32)
    span = torch.tensor(bnd[1] - bnd[0], dtype=F32)
    g = ((p - lo) / span) * 2.0 - 1.0
    f = ((g + 1.0) / 2.0) * float(n - 1)
    if border:
        f = torch.where(f.isnan(), torch.zeros_like(f), f).clamp(0.0, float(n - 1))
    return g, f


def taps(cfg, pts, border):
    """(g, f, inside) of points [..., 3]: fp32 normalised and tap coordinates, and the all(-1 <= g <= 1) mask."""
    gf = [axis_tap(pts[..., a], bnd, n, border) for a, (bnd, n) in enumerate(axes(cfg))]
    g = torch.stack([x[0] for x in gf], dim=-1)
    f = torch.stack([x[1] for x in gf], dim=-1)
    return g, f, ((g >= -1.0) & (g <= 1.0)).all(dim=-1)


def ref_sample(cfg, src, pts, border, mask):
    """The float64 gather: src [B, C, Z, Y, X] (float64; the activated volume where there is an activation), pts
    [B, P, 3] fp32 -> [B, C, P].  Floors from the fp32 tap coordinates, weights floor + 1 - f and f - floor in float64,
    eight taps, those that are no voxels skipped (not multiplied by zero), times the inside mask under mask_outside.
    What the kernel documents for a tap coordinate that is not finite, or 1e9 and beyond: no tap is a voxel (in
    border padding the clip has made it finite before)."""
    B, Cc, Z, Y, X = src.shape
    g, f, inside = taps(cfg, pts, border)
    dead = ~(f.isfinite() & (f.abs() < 1e9)).all(dim=-1, keepdim=True)
    f = torch.where(dead, torch.full_like(f, -5.0), f)
    fl = torch.floor(f)
    f, fl = f.double(), fl.double()
    w = (fl + 1.0 - f, f - fl)
    flat = src.reshape(B, Cc, -1)
    out = torch.zeros(B, Cc, pts.shape[1], dtype=F64)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        ix, iy, iz = fl[..., 0] + dx, fl[..., 1] + dy, fl[..., 2] + dz
        ok = (ix >= 0) & (ix <= X - 1) & (iy >= 0) & (iy <= Y - 1) & (iz >= 0) & (iz <= Z - 1)
        idx = ((iz.clamp(0, Z - 1) * Y + iy.clamp(0, Y - 1)) * X + ix.clamp(0, X - 1)).long()
        v = flat.gather(2, idx[:, None, :].expand(B, Cc, -1))
        wk = (w[dx][..., 0] * w[dy][..., 1] * w[dz][..., 2])[:, None, :]
        out = out + torch.where(ok[:, None, :], wk * v, torch.zeros((), dtype=F64))
    if mask:
        out = out * inside[:, None, :]
    return out


def records(cfg, pts, border, mask):
    """What sample_points_rank_kernel keeps: (active [B, P], floors [B, P, 3] int64, meaningful where active)."""
    g, f, inside = taps(cfg, pts, border)
    fl = torch.floor(f)
    n = torch.tensor([n for _, n in axes(cfg)], dtype=F32)
    act = ((fl >= -1.0) & (fl <= n - 1.0)).all(dim=-1)
    if mask:
        act = act & inside
    return act, torch.where(act[..., None], fl, torch.zeros_like(fl)).long()


def voxel_records(cfg, pts, border, mask):
    """[B, Z, Y, X] int64: the records the gather of each voxel walks -- the active points of its 2 x 2 x 2 cells."""
    act, fl = records(cfg, pts, border, mask)
    (_, X), (_, Y), (_, Z) = axes(cfg)
    B = pts.shape[0]
    cnt = torch.zeros(B, Z, Y, X, dtype=torch.int64)
    b = torch.arange(B)[:, None].expand(B, pts.shape[1])
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        ix, iy, iz = fl[..., 0] + dx, fl[..., 1] + dy, fl[..., 2] + dz
        ok = act & (ix >= 0) & (ix < X) & (iy >= 0) & (iy < Y) & (iz >= 0) & (iz < Z)
        cnt.index_put_((b[ok], iz[ok], iy[ok], ix[ok]), torch.ones((), dtype=torch.int64), accumulate=True)
    return cnt


# ---------------------------------------------------------------------------------------------------- the point set
def exact_coord(bnd, n, want_f, guess, want_g=None):
    """An fp32 coordinate within four ulps of `guess` whose tap coordinate is exactly want_f (and whose normalised
    coordinate is exactly want_g), or None."""
    p = np.float32(guess)
    cands, up, dn = [p], p, p
    for _ in range(4):
        up, dn = np.nextafter(up, np.float32(np.inf)), np.nextafter(dn, np.float32(-np.inf))
        cands += [up, dn]
    t = torch.tensor(np.array(cands, dtype=np.float32))
    g, f = axis_tap(t, bnd, n)
    hit = f == float(want_f)
    if want_g is not None:
        hit &= g == float(want_g)
    return float(t[hit][0]) if bool(hit.any()) else None


def hi_coord(bnd, n):
    """The fp32 coordinate on the high bound: g = 1 and f = n - 1 exactly; where fp32 has no such coordinate (p - lo
    rounds past the span either way: the size-1 x axis), the last one that is still inside."""
    c = exact_coord(bnd, n, n - 1, bnd[1], 1.0)
    if c is not None:
        return c
    p = np.float32(bnd[1])
    for _ in range(8):
        p = np.nextafter(p, np.float32(np.inf))
    assert float(axis_tap(torch.tensor(p), bnd, n)[0]) > 1.0
    for _ in range(32):
        p = np.nextafter(p, np.float32(-np.inf))
        if float(axis_tap(torch.tensor(p), bnd, n)[0]) <= 1.0:
            return float(p)
    raise AssertionError(bnd)


def to_ego(u, bnd, n):
    """Tap coordinate u (float64) -> ego coordinate; on a size-1 axis, where every tap coordinate is 0, u counts spans."""
    return bnd[0] + u * (bnd[1] - bnd[0]) / max(n - 1, 1)


# one spec per axis; a point's label is (kind, (spec x, spec y, spec z))
# (in voxels; on a size-1 axis in spans of the bound, so that the point is outside the bound all the same)
OUTSIDE = {"lo0.3": lambda n: -0.3, "lo0.9": lambda n: -0.9, "hi0.3": lambda n: max(n - 1, 1) + 0.3,
           "hi0.9": lambda n: max(n - 1, 1) + 0.9, "farlo": lambda n: -1.5, "farhi": lambda n: max(n - 1, 1) + 1.7}
EXTREME = {"+1e3": 1e3, "-1e3": -1e3, "+1e30": 1e30, "-1e30": -1e30, "nan": float("nan"), "+inf": float("inf"),
           "-inf": float("-inf")}
POINT_KINDS = ("interior", "centre", "bound", "out1", "out2", "out3", "far", "1e3", "1e30", "nonfinite")
N_NONFINITE = 6               # per sample: NaN, +inf, -inf, each in one coordinate and in all three


def structured_points(case, b):
    """The classes of one sample, crowds aside: [(kind, specs, (x, y, z))] in the order the P cases cut from -- one
    point of every label first (the low-corner point first of all), then the rest."""
    cfg = case.cfg
    ax = axes(cfg)
    gen = torch.Generator().manual_seed(7001 + 13 * b + 1000 * case.X + 100 * case.Y + 10 * case.Z)
    rnd = lambda: float(torch.rand((), generator=gen, dtype=F64))
    groups = []                                   # [(kind, specs, [points])]

    def coord(spec, a):
        bnd, n = ax[a]
        if spec == "in":                          # strictly inside a cell, a little off the voxels
            return to_ego((0.05 + 0.9 * rnd()) * (n - 1) if n > 1 else 0.05 + 0.9 * rnd(), bnd, n)
        if spec in OUTSIDE:
            return to_ego(OUTSIDE[spec](n), bnd, n)
        if spec in EXTREME:
            return EXTREME[spec]
        raise KeyError(spec)

    def add(kind, specs, count=1):
        groups.append((kind, specs, [tuple(coord(s, a) for a, s in enumerate(specs)) for _ in range(count)]))

    for d in ("0.3", "0.9"):                      # all three axes: the cells (-1, -1, -1) and (X-1, Y-1, Z-1)
        add("out3", ("lo" + d,) * 3)
        add("out3", ("hi" + d,) * 3)
    add("out3", ("lo0.3", "hi0.3", "lo0.9"))
    add("interior", ("in", "in", "in"), 300)
    # voxel centres: tap coordinates that are whole numbers on all three axes
    cen = []
    for bnd, n in ax:
        want = range(1, n - 1) if n > 2 else range(n)
        got = [exact_coord(bnd, n, i, to_ego(float(i), bnd, n)) for i in want]
        cen.append([c for c in got if c is not None])
    if all(cen):
        groups.append(("centre", ("ctr",) * 3, [tuple(c[(j * k) % len(c)] for c, k in zip(cen, (1, 3, 1))) for j in range(12)]))
    # exactly on lo and on hi of each axis (g = -1, g = 1), the other two axes inside
    for a, (bnd, n) in enumerate(ax):
        for side, c in (("onlo", exact_coord(bnd, n, 0, bnd[0], -1.0)), ("onhi", hi_coord(bnd, n))):
            specs = tuple(side if k == a else "in" for k in range(3))
            groups.append(("bound", specs, [tuple(c if k == a else coord("in", k) for k in range(3))]))
    groups.append(("bound", ("onhi",) * 3, [tuple(hi_coord(bnd, n) for bnd, n in ax)]))
    groups.append(("bound", ("onlo",) * 3, [tuple(exact_coord(bnd, n, 0, bnd[0], -1.0) for bnd, n in ax)]))
    for a in range(3):                            # one axis outside
        for s in ("lo0.3", "lo0.9", "hi0.3", "hi0.9"):
            add("out1", tuple(s if k == a else "in" for k in range(3)))
    for a, c in ((0, 1), (0, 2), (1, 2)):         # two axes outside: low-low, high-high, low-high
        for d in ("0.3", "0.9"):
            for sa, sc in (("lo", "lo"), ("hi", "hi"), ("lo", "hi")):
                add("out2", tuple(sa + d if k == a else (sc + d if k == c else "in") for k in range(3)))
    for s in ("farlo", "farhi"):                  # more than one voxel outside: no tap is a voxel
        add("far", (s, "in", "in"))
        add("far", (s,) * 3)
    add("far", ("in", "farhi", "lo0.3"))
    for kind in ("1e3", "1e30"):
        for sign in "+-":
            add(kind, ("in", sign + kind, "in"))
            add(kind, (sign + kind,) * 3)
    for a, s in enumerate(("nan", "+inf", "-inf") if b < 2 else ()):        # (12 per case: the first two samples)
        add("nonfinite", tuple(s if k == a else "in" for k in range(3)))
        add("nonfinite", (s,) * 3)
    first = [(k, s, p[0]) for k, s, p in groups]
    rest = [(k, s, q) for k, s, p in groups for q in p[1:]]
    return first + rest


def crowd_sites(case):
    """[(voxel (ix, iy, iz), records)]: kPtsHeavy exactly at an interior voxel (the light gather's last count), one more
    at voxel (0, 0, 0) (the heavy kernel's first), 600 at a second interior voxel.  The three 2 x 2 x 2 cell blocks are
    six voxels apart along the longest axis."""
    n = [case.X, case.Y, case.Z]
    a = n.index(max(n))
    assert n[a] >= 16
    mid = [min(2, m - 1) for m in n]
    s1, s2 = list(mid), list(mid)
    s1[a], s2[a] = 4, 10
    return [(tuple(s1), K_PTS_HEAVY), ((0, 0, 0), K_PTS_HEAVY + 1), (tuple(s2), 600)]


def crowd_points(case, b, pts, site, target):
    """Points in the support of voxel `site` that bring its records to `target`, counted with what is there already
    (pts [P, 3] of sample b).  Up to a voxel either side of the voxel on each axis -- which at voxel (0, 0, 0) reaches
    into the cells of floor -1 -- but inside the bounds where mask_outside would drop the point."""
    cfg = case.cfg
    have = int(voxel_records(cfg, pts[None], case.border, case.mask)[0, site[2], site[1], site[0]])
    need = target - have
    assert need > 0, (case.name, site, have, target)
    gen = torch.Generator().manual_seed(9001 + b + 17 * sum(site))
    u = torch.rand(need, 3, generator=gen, dtype=F64)
    cols = []
    for a, (bnd, n) in enumerate(axes(cfg)):
        lo, hi = site[a] - 0.98, site[a] + 0.98
        if n == 1:
            lo, hi = -0.9, 0.9                    # (every tap coordinate is 0; in spans of the bound)
        if case.mask:
            lo, hi = max(lo, 0.02), min(hi, max(n - 1, 1) - 0.02)
        cols.append(to_ego(lo + (hi - lo) * u[:, a], bnd, n))
    return torch.stack(cols, dim=-1).float()


@functools.lru_cache(maxsize=None)
def point_set(case):
    """(points [B, P, 3] fp32, labels [[(kind, specs) | ("crowd", site)] per point] per sample)."""
    per_b, labels = [], []
    for b in range(case.B):
        rows = structured_points(case, b)
        if case.P:
            rows = (rows * (case.P // len(rows) + 1))[:case.P] if case.P > len(rows) else rows[:case.P]
        pts = torch.tensor([r[2] for r in rows], dtype=F64).float().reshape(-1, 3)
        lab = [(r[0], r[1]) for r in rows]
        if not case.P:
            for site, target in crowd_sites(case):
                extra = crowd_points(case, b, pts, site, target)
                pts = torch.cat([pts, extra])
                lab += [("crowd", site)] * len(extra)
        per_b.append(pts)
        labels.append(lab)
    # the samples need different numbers of crowd points: the shorter ones are filled up with interior points between
    # the crowds' blocks (floors 6 and 7 on the longest axis), which changes no crowd's count
    P = max(len(p) for p in per_b)
    n = [case.X, case.Y, case.Z]
    a = n.index(max(n))
    for b in range(case.B):
        k = P - len(per_b[b])
        u = torch.rand(k, 3, generator=torch.Generator().manual_seed(5001 + b), dtype=F64) * 0.9 + 0.05
        cols = [to_ego(6.0 + 2.0 * u[:, c] if c == a else u[:, c] * (m - 1 if m > 1 else 1), bnd, m)
                for c, (bnd, m) in enumerate(axes(case.cfg))]
        per_b[b] = torch.cat([per_b[b], torch.stack(cols, dim=-1).float()])
        labels[b] += [("interior", ("in",) * 3)] * k
    return torch.stack(per_b), labels


@functools.lru_cache(maxsize=None)
def inputs(case):
    """CPU tensors of one case: volume [B, C, Z, Y, X] fp32 (bf16-rounded for a bf16 case; around the sdf bias where
    there is an activation), points [B, P, 3], grad_out [B, C, P], and the mask of the points with three finite
    coordinates."""
    pts, _ = point_set(case)
    gen = torch.Generator().manual_seed(31 + case.C + 7 * case.X + 11 * case.Y + 13 * case.Z + 17 * case.B)
    vol = torch.randn(case.B, case.C, case.Z, case.Y, case.X, generator=gen)
    if case.act:
        vol = 0.5 * vol - 1.0
    if case.bf16:
        vol = vol.bfloat16().float()
    gout = torch.randn(case.B, case.C, pts.shape[1], generator=gen)
    return types.SimpleNamespace(vol=vol, pts=pts, gout=gout, finite=pts.isfinite().all(dim=-1))


def reference(case, vol, pts, gout):
    """The float64 reference of one call: out, grad_volume, grad_beta and the sum of its terms' magnitudes (None
    without the sdf activation), A of the forward and of the backward (None with an activation), records per voxel."""
    cfg = case.cfg
    v = vol.double().requires_grad_(True)
    beta = terms = None
    src = v
    if case.act == "sdf":
        beta = torch.tensor(case.beta, dtype=F64, requires_grad=True)
        terms = beta.expand(v.shape)              # one term of d beta per voxel
        src = O.density_sdf(v, terms, cfg.sdf_bias)
    elif case.act:
        src = O.density_apply(v, case.act)
    out = ref_sample(cfg, src, pts, case.border, case.mask)
    g64 = gout.double()
    r = types.SimpleNamespace(out=out.detach(), gbeta=None, gscale=None, A_out=None, A_g=None,
                              nrec=voxel_records(cfg, pts, case.border, case.mask))
    if terms is not None:
        r.gvol, gt = torch.autograd.grad(out, [v, terms], g64)
        r.gbeta, r.gscale = float(gt.sum()), float(gt.abs().sum())
    else:
        (r.gvol,) = torch.autograd.grad(out, [v], g64, retain_graph=not case.act)
    if not case.act:
        (r.A_g,) = torch.autograd.grad(out, [v], g64.abs())
        r.A_out = ref_sample(cfg, vol.double().abs(), pts, case.border, case.mask)
    return r


@functools.lru_cache(maxsize=None)
def oracle(case):
    i = inputs(case)
    return reference(case, i.vol, i.pts, i.gout)


def ratio(err, allow):
    """max err / allow, an element with no allowance having to be exact."""
    q = torch.where(err == 0, torch.zeros_like(err), err / allow)
    return float(q.max()) if q.numel() else 0.0


def errors(case, got, ref, finite):
    """{what: (error, bar)} of one call's results against its reference.  Without an activation the bars are the derived
    ones, per element, and the error is the largest fraction of its bar an element uses; the points that are not finite
    are left out of this comparison in zeros padding and under mask_outside (non_finite_behaviour has them), and are
    compared in plain border padding, where the reference does what is documented for them."""
    out, gvol, gbeta = got
    keep = finite if (not case.border or case.mask) else torch.ones_like(finite)
    keep = keep[:, None, :].expand_as(ref.out)
    errs = {}
    d_out = (out.detach().cpu().double() - ref.out).abs()
    assert gvol.dtype == (torch.bfloat16 if case.bf16 else F32)
    g = gvol.detach().cpu().double()
    d_g = (g - ref.gvol).abs()
    gmax = float(ref.gvol.abs().max())
    if case.bf16:                                 # the fp32 gradient rounded once to bf16's 8-bit significand
        d_g = (d_g - BF16_GRAD_REL * ref.gvol.abs()).clamp_min(0)
    if case.act:
        errs["out"] = (float((d_out / (1 + ref.out.abs()))[keep].max()), ACT_OUT_BAR)
        errs["grad_volume"] = (float(d_g.max()) / (1 + gmax), ACT_GRAD_BAR)
        if ref.gbeta is not None:
            gb = float(gbeta)
            errs["grad_beta"] = (abs(gb - ref.gbeta) / max(ref.gscale, 1e-300), ACT_BETA_BAR)
        else:
            assert gbeta is None
        return errs
    allow = torch.minimum(K_FWD * U * ref.A_out, OUT_ATOL + OUT_RTOL * ref.out.abs())
    errs["out"] = (ratio(d_out[keep], allow[keep]), 1.0)
    n = ref.nrec[:, None].double()
    cap = torch.where(n > K_PTS_HEAVY, torch.full_like(n, GRAD_CAP_CROWD), torch.full_like(n, GRAD_CAP)) * gmax
    allow = torch.minimum((K_BWD_WEIGHT + n + K_BWD_TREE) * U * ref.A_g, cap.expand_as(ref.A_g))
    errs["grad_volume"] = (ratio(d_g, allow), 1.0)
    return errs


def non_finite_behaviour(case, out, finite):
    """What the kernel documents for points that are not finite: in zeros padding and under mask_outside their output is
    exactly 0 (and errors() has compared the gradients with a reference to which they add nothing); in plain border
    padding errors() has compared them with the reference, in which a NaN tap coordinate is 0 and +-inf is clipped."""
    assert int((~finite).sum()) <= 12, int((~finite).sum())
    if not case.border or case.mask:
        o = out.detach().cpu()
        sel = (~finite)[:, None, :].expand_as(o)
        assert bool((o[sel] == 0).all()), f"{case.name}: a non-finite point's output is not 0"
    assert bool(out.isfinite().all()), f"{case.name}: non-finite output"


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


_HOT = {}


def shared_hot(cfg, dev):
    """One HotPath per configuration for the whole sweep: its "sample" workspace is then reused across cases."""
    if (cfg, str(dev)) not in _HOT:
        _HOT[(cfg, str(dev))] = hot(cfg, dev)
    return _HOT[(cfg, str(dev))]


def run_gpu(hp, case, vol, pts, gout, dev, lattice=None, backward=True):
    """One forward (and backward): (out [B, C, P], grad_volume, grad_beta | None)."""
    v = vol.to(dev, torch.bfloat16 if case.bf16 else F32).requires_grad_(True)
    beta = torch.tensor(case.beta, device=dev, requires_grad=True) if case.act == "sdf" else None
    out = hp.sample_points(v, pts.to(dev), padding=case.padding, mask_outside=case.mask, activation=bool(case.act),
                           beta=beta, channel_last=case.channel_last, lattice=lattice)
    B, P = pts.shape[:2]
    assert out.shape == ((B, P, case.C) if case.channel_last else (B, case.C, P)) and out.dtype == F32
    if not backward:
        return out.permute(0, 2, 1) if case.channel_last else out, None, None
    g = gout.to(dev)
    out.backward(g.permute(0, 2, 1).contiguous() if case.channel_last else g)
    return (out.permute(0, 2, 1) if case.channel_last else out, v.grad, beta.grad if beta is not None else None)


def report(name, errs):
    for what, (e, b) in errs.items():
        print(f"SEEN {name} {what}: {e:.3e} (bar {b:.1e})")
    return [f"{name} {what}: {e:.3e} > {b:.1e}" for what, (e, b) in errs.items() if not e <= b]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_sample_points_sweep_against_float64(dev, case):
    """Outputs, the volume's gradient and grad_beta of every case against the float64 gather, and the documented
    behaviour of the points that are not finite."""
    i = inputs(case)
    got = run_gpu(shared_hot(case.cfg, dev), case, i.vol, i.pts, i.gout, dev)
    non_finite_behaviour(case, got[0], i.finite)
    bad = report(case.name, errors(case, got, oracle(case), i.finite))
    assert not bad, "\n".join(bad)


LATTICE = (7, 5, 11)          # P = 385: one full workgroup and a ragged one


@pytest.mark.gpu
def test_lattice_hint_changes_no_bit(dev):
    """The lattice hint only reorders the threads: with a matching (n0, n1, n2), and with one whose product is not P
    (ignored), the forward outputs are bit-equal to the call without a hint; occupancy_queries with bda_mat = None and
    B = 2 (the static grid, expanded) gives those bits as well, and they are the reference's to the bars."""
    n0, n1, n2 = LATTICE
    P = n0 * n1 * n2
    assert P % 256 != 0
    case = dataclasses.replace(BASE, name="lattice", padding="border")
    cfg = case.cfg
    hp = hot(cfg, dev)
    i = inputs(BASE)
    # a lattice that leaves the volume on every side, in the occ buffer's order (axis 0 outermost)
    lin = [torch.linspace(bnd[0] - 1.3, bnd[1] + 1.3, n, dtype=F64).float() for (bnd, _), n in zip(axes(cfg), LATTICE)]
    occ = torch.stack(torch.meshgrid(*lin, indexing="ij"), dim=-1)
    pts = occ.reshape(1, P, 3).expand(case.B, P, 3).contiguous()
    gout = i.gout[:, :, :P].contiguous()
    plain = run_gpu(hp, case, i.vol, pts, gout, dev)
    for hint in (LATTICE, (n0, n1, n2 + 1), (n2, n1, n0)):
        hinted = run_gpu(hp, case, i.vol, pts, gout, dev, lattice=hint)
        assert torch.equal(hinted[0], plain[0]), hint             # (the backward takes no hint, and the order of its
        #                                                             records, so its last bits, changes from run to run)
    zeros = dataclasses.replace(case, padding="zeros")
    plain0 = run_gpu(hp, zeros, i.vol, pts, gout, dev, backward=False)[0]
    assert torch.equal(run_gpu(hp, zeros, i.vol, pts, gout, dev, lattice=LATTICE, backward=False)[0], plain0)
    bad = report("lattice", errors(case, plain, reference(case, i.vol, pts, gout), torch.ones(case.B, P, dtype=torch.bool)))
    # occupancy_queries: semantic logits in border padding, the activated density in zeros padding, both hinted
    dens = inputs(CASE_BY_NAME["sdf+0.1"])
    beta = torch.tensor(0.1, device=dev)
    logits, density = hp.occupancy_queries(i.vol.to(dev), dens.vol.to(dev), occ.to(dev), None, beta)
    assert logits.shape == (case.B, case.C, *LATTICE) and density.shape == (case.B, 1, *LATTICE)
    assert torch.equal(logits.reshape(case.B, case.C, P), plain[0])
    act = dataclasses.replace(CASE_BY_NAME["sdf+0.1"], name="lattice-density")
    unhinted = run_gpu(hp, act, dens.vol, pts, gout[:, :1], dev, backward=False)[0]
    assert torch.equal(density.reshape(case.B, 1, P), unhinted)
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_workspace_reuse_keeps_the_low_corner_record(dev):
    """On one HotPath a large crowded call, then a small one with the low-corner point (P = 63: one point of every
    class): the first leaves records all over the "sample" workspace, and a key scheme that loses the low-corner
    record would have the gather of voxel (0, 0, 0) pick one of them up.  The small call's results are the reference's
    to the bars, as they are on a fresh HotPath, and the two forwards are bit-equal."""
    big, small = CASE_BY_NAME["C17"], dataclasses.replace(CASE_BY_NAME["P63"], C=17)
    assert big.cfg == small.cfg
    ib, i = inputs(big), inputs(small)
    act, fl = records(small.cfg, i.pts, False, False)
    assert bool((act & (fl == -1).all(dim=-1)).any())
    hp = hot(big.cfg, dev)
    run_gpu(hp, big, ib.vol, ib.pts, ib.gout, dev)
    used = run_gpu(hp, small, i.vol, i.pts, i.gout, dev)
    fresh = run_gpu(hot(small.cfg, dev), small, i.vol, i.pts, i.gout, dev)
    ref = reference(small, i.vol, i.pts, i.gout)
    bad = report("reused", errors(small, used, ref, i.finite)) + report("fresh", errors(small, fresh, ref, i.finite))
    assert not bad, "\n".join(bad)
    assert torch.equal(used[0], fresh[0])


@pytest.mark.gpu
def test_non_finite_voxel_behind_a_tap_that_is_no_voxel(dev):
    """inf in a face voxel, and zeros-padding points whose taps on that side are all outside the volume -- more than a
    voxel outside, +-1e3, NaN -- so that the forward clamps their addresses onto that voxel: aten skips such taps and
    gives 0; a forward that multiplies 0 * inf gives NaN.  Every other output is the reference's."""
    case = dataclasses.replace(BASE, name="inf-voxel")
    cfg = case.cfg
    i = inputs(BASE)
    vol = i.vol.clone()
    iy, iz = 3, 1
    vol[:, :, iz, iy, 0] = float("inf")
    (bx, X), (by, Y), (bz, Z) = axes(cfg)
    at = lambda ux, uy, uz: (to_ego(ux, bx, X), to_ego(uy, by, Y), to_ego(uz, bz, Z))
    extra = torch.tensor([at(-1.5, iy + 0.2, iz + 0.3), at(-1.5, iy - 0.8, iz - 0.7), (-1e3, at(0, iy + 0.5, 0)[1], at(0, 0, iz + 0.5)[2]),
                          (float("nan"), at(0, iy + 0.5, 0)[1], at(0, 0, iz + 0.5)[2])], dtype=F64).float()
    # no point of the set may have a tap that IS that voxel (its output would be inf by right)
    act, fl = records(cfg, i.pts, False, False)
    touches = act & (fl[..., 0] <= 0) & (fl[..., 1] >= iy - 1) & (fl[..., 1] <= iy) & (fl[..., 2] >= iz - 1) & (fl[..., 2] <= iz)
    pts = torch.stack([torch.cat([extra, i.pts[b][~touches[b]][:400]]) for b in range(case.B)])
    gout = i.gout[:, :, :pts.shape[1]].contiguous()
    out = run_gpu(hot(cfg, dev), case, vol, pts, gout, dev, backward=False)[0].detach().cpu()
    ref = ref_sample(cfg, vol.double(), pts, False, False)
    assert bool(ref.isfinite().all()) and bool((ref[:, :, :len(extra)] == 0).all())
    assert bool((out[:, :, :len(extra)] == 0).all()), out[:, :, :len(extra)]
    assert bool(out.isfinite().all())
    finite_vol = torch.where(vol.isfinite(), vol, torch.zeros_like(vol)).double().abs()
    allow = torch.minimum(K_FWD * U * ref_sample(cfg, finite_vol, pts, False, False), OUT_ATOL + OUT_RTOL * ref.abs())
    assert ratio((out.double() - ref).abs(), allow) <= 1.0


# ---------------------------------------------------------------------------------------------------- CPU
def test_cases_are_what_they_are_named_for():
    """axis_cells truncates: the volume of every case is the one intended; the axes hold the values of the sweep."""
    for c in CASES:
        cfg = c.cfg
        assert (cfg.vX, cfg.vY, cfg.vZ) == (c.X, c.Y, c.Z), c.name
        assert not c.act or c.C == 1, c.name
    assert (BASE.cfg.vZ, BASE.cfg.vY, BASE.cfg.vX, BASE.B, BASE.C, BASE.padding) == (5, 16, 16, 2, 5, "zeros")
    plain = [c for c in CASES if not (c.act or c.bf16 or c.border or c.mask or c.channel_last or c.P)]
    assert sorted({c.C for c in plain}) == CHANNELS
    assert {(c.C + 3) // 4 for c in plain} == set(range(1, 9))                       # every CP4 body
    assert all({4 * k, 4 * k - 3} <= {c.C for c in plain} for k in range(1, 9))      # ... full, and with three pad channels
    assert {c.X for c in plain} >= set(EXTENT_X) and {PVPB - 1, PVPB, PVPB + 1} <= set(EXTENT_X)
    assert {1} <= {c.Y for c in plain} and {1} <= {c.Z for c in plain} and {c.B for c in plain} == {1, 2, 3}
    assert {c.P for c in CASES} == {0, *POINTS}
    assert {(c.padding, c.mask, c.channel_last) for c in CASES if not c.act} == set(
        itertools.product(("zeros", "border"), (False, True), (False, True)))
    assert {(c.act, c.beta) for c in CASES if c.act and not (c.bf16 or c.border)} == {("sdf", 0.1), ("sdf", -0.1), ("sdf", 0.0), ("naive", 0.1)}
    assert {c.C for c in CASES if c.bf16 and not c.act} == {1, 5, 18}


def spec_holds(spec, p, g, f, n, bnd=None):
    """One axis of one point is where its label says (f, g: the unclipped fp32 tap and normalised coordinates)."""
    if spec in ("nan", "+inf", "-inf"):
        return {"nan": np.isnan(p), "+inf": p == np.inf, "-inf": p == -np.inf}[spec]
    if not np.isfinite(p):
        return False
    if spec in ("+1e3", "-1e3"):
        return p == float(spec) and (n == 1 or f < -1 or f >= n)
    if spec in ("+1e30", "-1e30"):
        return p == np.float32(float(spec)) and (n == 1 or abs(f) >= 1e9)
    if spec == "onlo":
        return f == 0 and g == -1
    if spec == "onhi":
        if f == n - 1 and g == 1:
            return True
        up = torch.tensor(np.nextafter(np.float32(p), np.float32(np.inf)))
        return (exact_coord(bnd, n, n - 1, bnd[1], 1.0) is None and g <= 1 and float(axis_tap(up, bnd, n)[0]) > 1
                and abs(f - (n - 1)) <= 1e-5 * n)
    if n == 1:                                    # a size-1 axis: every tap coordinate is 0; outside shows in g only
        return f == 0 and ((abs(g) <= 1) == (spec in ("in", "ctr")))
    fl = np.floor(f)
    if spec == "in":
        return 0 <= fl <= n - 2 and abs(g) <= 1
    if spec == "ctr":
        return f == fl and (0 < f < n - 1 if n > 2 else 0 <= f <= n - 1)
    if spec in ("lo0.3", "lo0.9"):
        return fl == -1 and abs(-f - float(spec[2:])) < 1e-3 and g < -1
    if spec in ("hi0.3", "hi0.9"):
        return fl == n - 1 and abs(f - (n - 1) - float(spec[2:])) < 1e-3 and g > 1
    return {"farlo": fl < -1, "farhi": fl > n - 1}[spec]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_point_set_covers_every_class(case):
    """From the reference's fp32 floors and per-cell counts, for every case: each point is where its label says; every
    class of POINT_KINDS has at least one point (a P case: as many labels as fit, the low-corner point first); the
    cells (-1, -1, -1) and (X-1, Y-1, Z-1) are hit where all three axes have more than one voxel; the bounds count as
    inside; the three crowds bring their voxels to exactly 256, 257 and 600 records, the first staying on the light
    path, the 257 at voxel (0, 0, 0) in zeros padding fed partly out of the low-corner cell; at most 12 points are not
    finite."""
    cfg = case.cfg
    pts, labels = point_set(case)
    ns = [n for _, n in axes(cfg)]
    g, f, inside = taps(cfg, pts, False)
    assert pts.shape[0] == case.B and (not case.P or pts.shape[1] == case.P)
    assert int((~pts.isfinite().all(dim=-1)).sum()) <= 12
    for b in range(case.B):
        kinds = set()
        for p, (kind, specs) in enumerate(labels[b]):
            kinds.add(kind)
            if kind == "crowd":
                continue
            for a in range(3):
                assert spec_holds(specs[a], float(pts[b, p, a]), float(g[b, p, a]), float(f[b, p, a]), ns[a], axes(cfg)[a][0]), \
                    (case.name, b, p, kind, specs, a, pts[b, p].tolist(), f[b, p].tolist())
            if kind in ("interior", "centre", "bound"):
                assert bool(inside[b, p]), (case.name, kind, specs)
        all_labels = {(k, s) for k, s, _ in structured_points(case, b)}
        here = set(POINT_KINDS) - ({"nonfinite"} if b >= 2 else set())
        assert {k for k, _ in all_labels} == here, case.name
        for a in range(3):
            for side in ("onlo", "onhi"):
                assert any(k == "bound" and s[a] == side and s.count(side) == 1 for k, s in all_labels), (case.name, a, side)
        assert sum(k == "nonfinite" for k, _ in all_labels) == (N_NONFINITE if b < 2 else 0)
        if case.P:
            want = min(case.P, len(all_labels))
            assert len(set(labels[b][:want])) == want and labels[b][0] == ("out3", ("lo0.3",) * 3), case.name
            continue
        assert kinds == here | {"crowd"} and set(labels[b]) >= all_labels, case.name
    act0, fl0 = records(cfg, pts, False, False)                   # zeros padding, no mask: the positions themselves
    if min(ns) > 1:
        lo = act0 & (fl0 == -1).all(dim=-1)
        hi = act0 & (fl0 == torch.tensor([n - 1 for n in ns])).all(dim=-1) & (f > torch.tensor([n - 1.0 for n in ns])).all(dim=-1)
        assert bool(lo.any(dim=1).all()) and (bool(hi.any(dim=1).all()) or case.P == 1), case.name
    if case.P:
        return
    nrec = voxel_records(cfg, pts, case.border, case.mask)
    (s1, t1), (s0, t0), (s2, t2) = crowd_sites(case)
    for b in range(case.B):
        at = lambda s: int(nrec[b, s[2], s[1], s[0]])
        assert (at(s1), at(s0), at(s2)) == (K_PTS_HEAVY, K_PTS_HEAVY + 1, 600) == (t1, t0, t2), (case.name, b)
        # the light gather's last count is the largest around its voxel: nothing near it goes to the heavy kernel
        z, y, x = (slice(max(s1[k] - 1, 0), s1[k] + 2) for k in (2, 1, 0))
        assert int(nrec[b, z, y, x].max()) == K_PTS_HEAVY, case.name
        assert s1 != (0, 0, 0) and s2 != (0, 0, 0) and all(0 < s2[k] < ns[k] - 1 or ns[k] <= 2 for k in range(3))
    assert int((nrec > K_PTS_HEAVY).sum()) >= 2 * case.B
    if not case.border and not case.mask and min(ns) > 1:
        act, fl = records(cfg, pts, False, False)
        corner = act & (fl == -1).all(dim=-1)
        crowd = torch.tensor([[k == "crowd" for k, _ in lab] for lab in labels])
        assert bool((corner & crowd).any(dim=1).all()) and bool((~corner & crowd).any(dim=1).all()), case.name


def test_low_corner_records_pack_to_key_zero():
    """Why the base case needs the KEY buffer's own sentinel: its point set holds active points (zeros padding, no
    mask) whose packed cell key (ix0 + 1) | (iy0 + 1) << 11 | (iz0 + 1) << 22 is 0 -- floors (-1, -1, -1), counted into
    cell 0 and walked by the gather of voxel (0, 0, 0).  A fill that returns on key == 0 never writes their records,
    and that gather reads whatever the slot held: with 0 for "inactive" the sweep's base case cannot pass.  The
    committed fixtures held no such point."""
    pts, labels = point_set(BASE)
    act, fl = records(BASE.cfg, pts, False, False)
    key = (fl[..., 0] + 1) | ((fl[..., 1] + 1) << 11) | ((fl[..., 2] + 1) << 22)
    lost = act & (key == 0)
    assert int(lost.sum()) >= 2 * BASE.B + 10                      # the out3 points, and an eighth of the corner crowd
    assert bool((fl[lost] == -1).all())
    assert bool((key[act] >= 0).all()) and bool((key[act & ~lost] > 0).all())   # bit 31 is free for the sentinel
    # each of them carries weight (fx + 1)(fy + 1)(fz + 1) > 0 to voxel (0, 0, 0): the reference does contribute
    _, f, _ = taps(BASE.cfg, pts, False)
    assert bool(((f[lost] + 1).prod(dim=-1) > 0).all())
    r = oracle(BASE)
    assert int(r.nrec[0, 0, 0, 0]) == K_PTS_HEAVY + 1 and float(r.A_g[:, :, 0, 0, 0].min()) > 0


PINNED = ["base", "border", "zeros-mask", "border-mask", "X1", "Y1", "Z1", "X33", "sdf+0.1", "naive", "P63"]


@pytest.mark.parametrize("name", PINNED)
def test_reference_is_aten_in_float64(name):
    """The gather above against aten: on the finite points it equals O.sample_points(volume.double(), ...) on the same
    fp32-rounded tap coordinates -- handed over as float64 normalised coordinates g' = 2 f / (n - 1) - 1, which aten
    unnormalises in float64 to f (1 + e), a handful of 2^-53 roundings -- in outputs and gradients, with that
    unnormalisation's slack: the ulp of the coordinate times the largest difference between neighbours (the zero padding
    counting as a neighbour).  The fp32 normalised coordinates, from which the inside mask comes, are the oracle's
    bits."""
    case = CASE_BY_NAME[name]
    cfg, i = case.cfg, inputs(case)
    bounds = (cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg)
    pts = torch.stack([i.pts[b][i.finite[b]] for b in range(case.B)])
    g, f, inside = taps(cfg, pts, False)
    assert torch.equal(g, O.normalise_points(pts, bounds))
    ns = torch.tensor([n for _, n in axes(cfg)], dtype=F64)
    gd = torch.where(ns > 1, f.double() / (ns - 1).clamp_min(1) * 2.0 - 1.0, torch.zeros((), dtype=F64))
    unit = ((-1.0, 1.0, 1.0),) * 3
    v = i.vol.double().requires_grad_(True)
    src = v if not case.act else O.density_apply(v, case.act, torch.tensor(case.beta, dtype=F64), cfg.sdf_bias)
    mine = ref_sample(cfg, src, pts, case.border, case.mask)
    aten = O.sample_points(src, gd, unit, case.padding, False)
    if case.mask:
        aten = aten * inside[:, None, :]
    s = src.detach()
    diff = max([float(s.abs().max())] + [float((s.narrow(d, 1, s.shape[d] - 1) - s.narrow(d, 0, s.shape[d] - 1)).abs().max())
                                         for d in (2, 3, 4) if s.shape[d] > 1])
    # |f' - f| <= 8 * 2^-53 (|f| + n) per axis (the roundings of g' and of aten's (g' + 1) / 2 * (n - 1)); a point
    # further out than 1e6 has the same taps on both sides whatever its last bits
    near = f.abs() < 1e6
    df = torch.where(near, 8 * 2.0 ** -53 * (f.double().abs() + ns), torch.zeros((), dtype=F64)).sum(dim=-1)
    slack = df * diff
    assert bool(((mine - aten).abs() <= slack[:, None, :]).all()), float((mine - aten).abs().max())
    assert float((mine - aten).detach().abs().max()) <= 1e-12
    gout = i.gout[:, :, :pts.shape[1]].double()
    (gm,) = torch.autograd.grad(mine, [v], gout, retain_graph=True)
    (ga,) = torch.autograd.grad(aten, [v], gout)
    # a weight moves by at most the three axes' |f' - f|; a voxel's gradient by that times sum |grad_out| (times the
    # activation's largest slope, 1 / (2 beta^2) for the sdf density at beta = 0.1)
    slope = 1.0 if not case.act else 51.0
    lim = float(df.max()) * float(gout.abs().sum()) * slope
    assert float((gm - ga).abs().max()) <= lim, (float((gm - ga).abs().max()), lim)
    assert lim < 1e-6                             # (far below any fp32 bar)


def test_non_finite_points_in_the_reference():
    """The reference does for the points that are not finite what sample_points.hip documents: in zeros padding and under
    mask_outside they give 0 and add nothing to the gradient (the gradient is that of the set without them); in border
    padding a NaN coordinate acts as tap coordinate 0 and +-inf as the face it is clipped to -- the reference on the
    points with lo, hi, lo written in their place."""
    for name in ("base", "border", "zeros-mask", "border-mask"):
        case = CASE_BY_NAME[name]
        cfg, i = case.cfg, inputs(case)
        assert int((~i.finite).sum()) == N_NONFINITE * case.B == 12
        v = i.vol.double().requires_grad_(True)
        out = ref_sample(cfg, v, i.pts, case.border, case.mask)
        (gv,) = torch.autograd.grad(out, [v], i.gout.double())
        bad = (~i.finite)[:, None, :].expand_as(out)
        if case.border and not case.mask:
            lo = torch.tensor([b[0] for b, _ in axes(cfg)], dtype=F32)
            hi = torch.tensor([hi_coord(b, n) for b, n in axes(cfg)], dtype=F32)
            sub = torch.where(i.pts.isnan() | (i.pts == -np.inf), lo, torch.where(i.pts == np.inf, hi, i.pts))
            assert bool(sub.isfinite().all())
            out2 = ref_sample(cfg, v, sub, True, False)
            assert torch.equal(out2, out) and bool((out[bad] != 0).any())
            continue
        assert bool((out[bad] == 0).all())
        keep = torch.stack([i.pts[b][i.finite[b]] for b in range(case.B)])
        gk = torch.stack([i.gout[b][:, i.finite[b]] for b in range(case.B)]).double()
        (gv2,) = torch.autograd.grad(ref_sample(cfg, v, keep, case.border, case.mask), [v], gk)
        assert torch.equal(gv2, gv)


def sample_desc(C_=5, activation=0):
    d = _capi.VampSampleDesc()
    d.B, d.C, d.Z, d.Y, d.X = 2, C_, 5, 16, 16
    for a, (bnd, _) in enumerate(axes(BASE.cfg)):
        d.lo[a], d.span[a] = bnd[0], bnd[1] - bnd[0]
    d.padding, d.in_dtype, d.activation = _capi.VAMP_PAD_ZEROS, _capi.VAMP_F32, activation
    d.density_mode, d.sdf_bias, d.beta_min = _capi.VAMP_DENSITY_SDF_LAPLACE, -1.0, 1e-4
    return d


def test_refusals_need_no_pointer():
    """C = 33 and an activation on C = 2 are refused by the descriptor alone: validate runs before any pointer is read
    (every pointer here is NULL), forward and backward, through the checked binding, which raises the message."""
    from vampire_amd.build import build_library
    build_library(verbose=False)
    lib = _capi.checked()
    for d, msg in ((sample_desc(MAX_C + 1), "0 < C <= 32"), (sample_desc(2, activation=1), "1-channel volume")):
        with pytest.raises(_capi.VampireHipError, match=msg):
            lib.vamp_sample_points_forward(C.byref(d), None, None, None, 4, None, None)
        with pytest.raises(_capi.VampireHipError, match=msg):
            lib.vamp_sample_points_backward(C.byref(d), None, None, None, 4, None, None, None, None, 0, None)
    # ... and C = 32 with the same NULLs gets past validate, to the pointer check
    with pytest.raises(_capi.VampireHipError, match="null pointer"):
        lib.vamp_sample_points_forward(C.byref(sample_desc(MAX_C)), None, None, None, 4, None, None)


def test_constants_are_the_kernels():
    """The constants the point set is built around are still those of the source."""
    import os
    from conftest import ROOT
    text = " ".join(open(os.path.join(ROOT, "vampire_amd", "csrc", "sample_points.hip")).read().split())
    for line in ("constexpr int kPtsHeavy = 256;", "constexpr int PGL = 8;", "constexpr int PVPB = 256 / PGL;",
                 "if (vox_ok && cr.tot > kPtsHeavy) {", "d->C > 0 && d->C <= 32",
                 "KEY[gid] = act ? key : -1;", "if (key < 0) return;"):
        assert line in text, line
