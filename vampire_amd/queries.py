"""The four point queries of a step as one operator (Python over the C ABI): the lidar points' semantic logits and sdf
and the Occ3D grid's logits and density of base_vampire2.py:576-609 from packed points with per-sample counts
(vamp_point_queries_forward / _backward, csrc/point_queries.hip).  One autograd node: one forward launch per point set
and one backward that builds one cell list and writes each volume's gradient once.  `HotPath.point_queries` is the
public entry; there is no CPU fallback."""
import collections

import torch

from . import _capi
from ._tensors import _accept_float, _chk, _density_code, _dtype_code, _pad_samples, _scalar, _stream

PointQueries = collections.namedtuple("PointQueries", "pts_logits pts_sdf occ_logits occ_density")

MAX_ROW = 32          # the backward's widest gradient row: K semantic channels + the density channel


def point_queries_supported(B, K, Z, Y, X, M=0, P_occ=0):
    """What vamp_point_queries_supported answers for these shapes (valid bounds, dtypes and density mode taken for
    granted), without the library."""
    if not (B > 0 and K > 0 and K + 1 <= MAX_ROW):
        return False
    if not (0 < Z < 511 and 0 < Y < 2047 and 0 < X < 2047):
        return False
    if M < 0 or P_occ < 0 or B * (M + 2 * P_occ) >= 0x7fffffff:
        return False
    ncell = (B * (Z + 1) * (Y + 1) * (X + 1) + 2 + 2047) // 2048 * 2048
    return B * Z * Y * X < 0x7fffffff and ncell < 0x7fffffff


def query_desc(cfg, B, K, sem_code, den_code, M, want_sdf, P_occ, occ_shared, lattice=None) -> _capi.VampQueryDesc:
    """The descriptor of `cfg`'s seg volume for these point sets; host only."""
    d = _capi.VampQueryDesc()
    d.B, d.K, d.Z, d.Y, d.X = B, K, cfg.vZ, cfg.vY, cfg.vX
    for i, bnd in enumerate((cfg.x_bound_seg, cfg.y_bound_seg, cfg.z_bound_seg)):
        d.lo[i] = bnd[0]
        d.span[i] = bnd[1] - bnd[0]
    d.density_mode = _density_code(cfg)
    d.sdf_bias, d.beta_min = cfg.sdf_bias, 1e-4
    d.sem_dtype, d.den_dtype = sem_code, den_code
    d.M, d.want_sdf, d.P_occ, d.occ_shared = M, 1 if want_sdf else 0, P_occ, 1 if occ_shared else 0
    for i in range(3):
        d.lattice[i] = int(lattice[i]) if lattice is not None else 0
    return d


def _device_tensor(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise _capi.VampireHipError(f"{name} must be a device tensor (no CPU fallback)")
    return t


def point_queries(hp, semantic_logits, density_feature, beta=None, *, points=None, counts=None, sdf=False,
                  occ_points=None, lattice=None):
    """See HotPath.point_queries.  Every mistake of the caller's raises here, before the first library call."""
    c = hp.cfg
    _device_tensor(semantic_logits, "semantic_logits")
    if semantic_logits.dim() != 5:
        raise ValueError(f"semantic_logits: expected [B, K, Z, Y, X], got {tuple(semantic_logits.shape)}")
    B, K = semantic_logits.shape[:2]
    _chk(_accept_float(semantic_logits, "semantic_logits"), (B, K, c.vZ, c.vY, c.vX), "semantic_logits")
    if density_feature is None:
        if sdf or occ_points is not None:
            raise ValueError("pts_sdf and the occupancy queries read density_feature: it is missing")
    else:
        _device_tensor(density_feature, "density_feature")
        _chk(_accept_float(density_feature, "density_feature"), (B, 1, c.vZ, c.vY, c.vX), "density_feature")
    if K + 1 > MAX_ROW:
        raise ValueError(f"semantic_logits: K = {K} channels, the operator takes K + 1 <= {MAX_ROW}")
    if points is None:
        if counts is not None:
            raise ValueError("counts without points")
    elif isinstance(points, torch.Tensor):
        _device_tensor(points, "points")
        if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 3:
            raise ValueError(f"points: expected shape ({B}, M, 3), got {tuple(points.shape)}")
        if counts is not None:
            _device_tensor(counts, "counts")
            if counts.dtype != torch.int32 or tuple(counts.shape) != (B,):
                raise ValueError(f"counts must be int32 [{B}], got {counts.dtype} {tuple(counts.shape)}")
    else:
        if counts is not None:
            raise ValueError("counts belongs to packed points: per-sample lists carry their own lengths")
        points = list(points)
        if len(points) != B:
            raise ValueError(f"{len(points)} point tensors for {B} samples")
        for p in points:
            _device_tensor(p, "points")
            if p.dim() != 2 or p.shape[1] != 3:
                raise ValueError(f"every sample needs points [n, 3], got {tuple(p.shape)}")
        points, counts = _pad_samples([p.float() for p in points])
    if occ_points is not None:
        _device_tensor(occ_points, "occ_points")
        if occ_points.dim() != 3 or occ_points.shape[0] not in (1, B) or occ_points.shape[2] != 3:
            raise ValueError(f"occ_points: expected shape ({B} | 1, P, 3), got {tuple(occ_points.shape)}")
        if lattice is not None and (len(lattice) != 3 or lattice[0] * lattice[1] * lattice[2] != occ_points.shape[1]):
            raise ValueError(f"lattice {tuple(lattice)} does not hold the {occ_points.shape[1]} occupancy points")
    if not point_queries_supported(B, K, c.vZ, c.vY, c.vX, 0 if points is None else points.shape[1],
                                   0 if occ_points is None else occ_points.shape[1]):
        raise ValueError("point_queries: shapes outside the operator's limits (point_queries_supported)")
    if beta is None:
        if occ_points is not None and c.density_mode == "sdf":
            raise ValueError("density_mode='sdf' needs the beta parameter")
        beta = torch.zeros((), device=hp.device)
    else:
        _scalar(beta, "beta")
    with torch.cuda.device(hp.device):
        out = _PointQueriesFn.apply(hp, semantic_logits, density_feature, beta, points, counts, occ_points,
                                    bool(sdf), None if lattice is None else tuple(lattice))
    return PointQueries(*out)


class _PointQueriesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hp, semantic, density, beta, points, counts, occ_points, sdf, lattice):
        c = hp.cfg
        B, K = semantic.shape[:2]
        ctx.sem_dtype, ctx.den_dtype = semantic.dtype, None if density is None else density.dtype
        semantic = _chk(_accept_float(semantic, "semantic_logits"), (B, K, c.vZ, c.vY, c.vX), "semantic_logits")
        if density is not None:
            density = _chk(_accept_float(density, "density_feature"), (B, 1, c.vZ, c.vY, c.vX), "density_feature")
        dev = semantic.device
        M = 0 if points is None else points.shape[1]
        P = 0 if occ_points is None else occ_points.shape[1]
        if points is not None:
            points = _chk(points.float(), (B, M, 3), "points")
        if counts is not None:
            counts = counts.contiguous()
        shared = occ_points is not None and occ_points.shape[0] == 1 and B > 1
        if occ_points is not None:
            occ_points = occ_points.float().contiguous()
        d = query_desc(c, B, K, _dtype_code(semantic), _dtype_code(density) if density is not None else _capi.VAMP_F32,
                       M, sdf, P, shared, lattice)
        ctx.beta_shape = beta.shape
        beta = _scalar(beta, "beta")
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        pts_logits = new(B, M, K) if points is not None else None
        pts_sdf = new(B, M) if points is not None and sdf else None
        occ_logits = new(B, K, P) if occ_points is not None else None
        occ_density = new(B, 1, P) if occ_points is not None else None
        hp.vamp.vamp_point_queries_forward(d, semantic, density, beta, points, counts, occ_points, pts_logits, pts_sdf,
                                           occ_logits, occ_density, _stream())
        ctx.hp, ctx.desc, ctx.sem_shape = hp, d, semantic.shape
        ctx.has = (density is not None, points is not None, counts is not None, occ_points is not None)
        ctx.save_for_backward(*[t for t in (density, points, counts, occ_points) if t is not None], beta)
        return pts_logits, pts_sdf, occ_logits, occ_density

    @staticmethod
    def backward(ctx, g_pts_logits, g_pts_sdf, g_occ_logits, g_occ_density):
        hp, d = ctx.hp, ctx.desc
        saved = list(ctx.saved_tensors)
        beta = saved.pop()
        density, points, counts, occ_points = (saved.pop(0) if have else None for have in ctx.has)
        dev = beta.device
        up = [None if g is None else g.contiguous().float()
              for g in (g_pts_logits, g_pts_sdf, g_occ_logits, g_occ_density)]
        gsem = torch.empty(ctx.sem_shape, dtype=torch.float32, device=dev)
        gden = torch.empty(density.shape, dtype=torch.float32, device=dev) if density is not None else None
        sdf_beta = density is not None and occ_points is not None and hp.cfg.density_mode == "sdf"
        gbeta = torch.zeros(1, dtype=torch.float32, device=dev) if sdf_beta else None
        ws = hp._workspace("queries", hp.vamp.vamp_point_queries_workspace_bytes(d))
        hp.vamp.vamp_point_queries_backward(d, density, beta, points, counts, occ_points, *up, gsem, gden, gbeta,
                                            ws, ws.numel(), _stream())
        return (None, gsem.to(ctx.sem_dtype), None if gden is None else gden.to(ctx.den_dtype),
                gbeta.reshape(ctx.beta_shape) if sdf_beta else None, None, None, None, None, None)
