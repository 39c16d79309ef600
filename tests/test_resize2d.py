"""The 2-D bilinear resize of the rendered maps (vampire_amd/csrc/resize2d.hip; layers.resize_bilinear2d and
resize_bilinear2d_pack; SWITCHES.resize2d in the backbone) against an oracle of its own.

Oracle: the taps and weights in numpy float32 by aten's chain (scale = (in - 1) / (out - 1), src = scale * o,
i0 = (int) src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1), then the blend (forward) or the transposed sum
(backward) in float64 with those fp32 weights, so that only the kernel's own arithmetic is left to bound.

Bounds, per element, from operation counts (u = 2^-24):
  forward   |err| <= 8 u sum |w v| over the four taps: every term passes four roundings (w0 * a, the inner add, the
            product with the row weight, the outer add); a factor 2 over that.
  backward  |err| <= (n + 4) u sum |w g|, n = contributions to the element (taps with a nonzero weight).  The kernel
            sums nx outputs along x and ny rows along y (n = nx ny): a term passes at most nx + ny + 1 roundings (its
            product with the column weight and nx - 1 adds, the product with the row weight and ny - 1 adds, one more
            add where both taps of the last source row fall on it), and nx + ny + 1 <= nx ny + 4 for all nx, ny >= 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from vampire_amd import _capi
from test_hip_parity import close, dev  # noqa: F401  (dev: the module-scoped device fixture)

U = 2.0 ** -24
BAND, COLS, GROUP = _capi.VAMP_RESIZE2D_BAND_ROWS, _capi.VAMP_RESIZE2D_COL_CHUNK, _capi.VAMP_RESIZE2D_PLANE_GROUP
CHUNK, STRIP_MAX, MAX_RUN = _capi.VAMP_RESIZE2D_STRIP_CHUNK, _capi.VAMP_RESIZE2D_STRIP_MAX, _capi.VAMP_RESIZE2D_MAX_RUN


# ------------------------------------------------------------------------------------------------ the oracle
def axis_scale(n_in, n_out):
    return np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)


def taps(n_in, n_out):
    """(i0, i1, l0, l1) of every output index, in float32 as the kernels compute them."""
    src = axis_scale(n_in, n_out) * np.arange(n_out, dtype=np.float32)
    assert src.dtype == np.float32
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l0, l1


def weight_matrix(n_in, n_out):
    """W [out, in] float64 with the fp32 weights (both taps of an output add up where they meet), and the number of
    taps with a nonzero weight per source index."""
    i0, i1, l0, l1 = taps(n_in, n_out)
    w = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    np.add.at(w, (o, i0), l0.astype(np.float64))
    np.add.at(w, (o, i1), l1.astype(np.float64))
    cnt = np.zeros(n_in, dtype=np.int64)
    np.add.at(cnt, i0[l0 != 0], 1)
    np.add.at(cnt, i1[l1 != 0], 1)
    return w, cnt


def oracle_forward(x, oh, ow):
    """x [P, ih, iw] float32 -> (out float64, bound): aten's nesting with fp32 weights, float64 arithmetic."""
    x = x.astype(np.float64)
    y0, y1, h0, h1 = taps(x.shape[1], oh)
    x0, x1, w0, w1 = taps(x.shape[2], ow)
    h0, h1 = h0.astype(np.float64)[None, :, None], h1.astype(np.float64)[None, :, None]
    w0, w1 = w0.astype(np.float64)[None, None, :], w1.astype(np.float64)[None, None, :]
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    c, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    out = h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d)
    mag = h0 * (w0 * np.abs(a) + w1 * np.abs(b)) + h1 * (w0 * np.abs(c) + w1 * np.abs(d))
    return out, 8 * U * mag


def oracle_backward(g, ih, iw):
    """g [P, oh, ow] float32 -> (grad_in float64, bound): the transposed sum with the fp32 weights."""
    g = g.astype(np.float64)
    wy, cy = weight_matrix(ih, g.shape[1])
    wx, cx = weight_matrix(iw, g.shape[2])
    gin = wy.T @ g @ wx
    mag = wy.T @ np.abs(g) @ wx
    n = cy[:, None] * cx[None, :]
    return gin, (n[None] + 4) * U * mag


def worst(got, ref, bound):
    """(largest error, largest error / bound over the elements with a bound)."""
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err[bound == 0] == 0)
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    return float(err.max()), ratio


# --------------------------------------------------------------- Python mirror of the launcher's host logic
def first_at_least(scale, n_out, v):
    """resize2d.hip first_at_least: the first output whose i0 is >= v, in float32."""
    if v <= 0:
        return 0
    o = 0
    if scale > 0:
        e = np.float32(v) / scale - np.float32(2)
        o = (int(e) if e < np.float32(n_out) else n_out) if e > 0 else 0
    while o > 0 and int(scale * np.float32(o - 1)) >= v:
        o -= 1
    while o < n_out and int(scale * np.float32(o)) < v:
        o += 1
    return o


def run_fits(n_in, n_out, hits):
    return n_out <= hits if n_in == 1 else 2 * (n_out - 1) // (n_in - 1) + 2 <= hits


def strip_fits(iw, ow):
    s = axis_scale(iw, ow)
    for x0 in range(0, iw, COLS):
        x1 = min(iw, x0 + COLS)
        ob, oe = first_at_least(s, ow, x0 - 1) & ~3, first_at_least(s, ow, x1)
        if (oe - ob + 3) // 4 * 4 > STRIP_MAX:
            return False
    return True


def supported(ih, iw, oh, ow):
    if min(ih, iw, oh, ow) <= 0 or ih * iw >= 2 ** 31 - 1 or oh * ow >= 2 ** 31 - 1:
        return 0
    return int(run_fits(iw, ow, MAX_RUN) and strip_fits(iw, ow))


# forward + backward cases: (planes, ih, iw, oh, ow)
CASES = {
    "x4 vector stores": (3, 4, 44, 16, 176),
    "x4 scalar tail 27": (2, 5, 7, 20, 27),
    "x4 scalar tail 19x28": (2, 5, 7, 19, 28),
    "band - 1": (1, BAND - 1, 6, 4 * BAND - 4, 24),
    "band + 1": (1, BAND + 1, 6, 4 * BAND + 4, 24),
    "two bands + 1": (1, 2 * BAND + 1, 5, 8 * BAND + 3, 20),
    "strip chunk - 1": (1, 3, 64, 6, CHUNK - 1),
    "strip chunk + 1": (1, 3, 64, 6, CHUNK + 1),
    "strip chunk - 4": (1, 3, 64, 6, CHUNK - 4),
    "strip chunk + 4": (1, 3, 64, 6, CHUNK + 4),
    "column chunk - 1": (1, 2, COLS - 1, 4, 4 * COLS - 4),
    "column chunk + 1": (1, 2, COLS + 1, 4, 4 * COLS + 4),
    "column chunk + 1 scalar": (1, 2, COLS + 1, 3, 2 * COLS + 1),
    "one row": (2, 1, 9, 4, 36),
    "one column": (2, 6, 1, 24, 1),
    "identity": (2, 8, 12, 8, 12),
    "out 1 along y": (2, 5, 7, 1, 28),
    "out 1 along x": (2, 5, 7, 20, 1),
    "longest run": (1, 2, 2, 8, 8),
    # 16-byte stores at ratios between 1 and 4: the forward's three-column path, whose last output of a row sits on
    # the last source column (i0 == i1 == iw - 1, two columns from the group's first tap), and the general path (x1.5)
    "x2 vector stores": (2, 8, 8, 16, 16),
    "x2 vector stores 4 -> 8": (2, 4, 4, 8, 8),
    "x2.4 vector stores": (2, 5, 5, 12, 12),
    "x2.7 vector stores": (2, 15, 15, 40, 40),
    "x3 vector stores": (2, 6, 12, 18, 36),
    "x1.5 vector stores": (2, 8, 8, 12, 12),
    "x2 module shape": (3, 16, 44, 32, 88),
    "down 16 -> 8": (2, 16, 16, 8, 8),
    "down 9x13 -> 4x6": (2, 9, 13, 4, 6),
    "down 256 -> 128": (2, 256, 256, 128, 128),
}
REFUSED = (4, 4, 4, 40)


def case_inputs(name):
    """`name`: a key of CASES, or a (planes, ih, iw, oh, ow) of the caller's own (tests/test_step_kernels_sweep.py)."""
    p, ih, iw, oh, ow = CASES[name] if isinstance(name, str) else name
    rng = np.random.default_rng(abs(hash((p, ih, iw, oh, ow))) % 2 ** 32)
    return (rng.standard_normal((p, ih, iw)).astype(np.float32), rng.standard_normal((p, oh, ow)).astype(np.float32))


# =============================================================================================== CPU tests
@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def test_oracle_is_bilinear_align_corners():
    """The oracle is F.interpolate(mode='bilinear', align_corners=True): within 1e-4 max|x| of the float64 aten result on
    every test shape (the fp32 weights differ from float64 ones by about 2e-5 at src near 175), and its backward is the
    transpose of its forward."""
    for name in CASES:
        x, g = case_inputs(name)
        oh, ow = g.shape[1:]
        out, _ = oracle_forward(x, oh, ow)
        ref = F.interpolate(torch.from_numpy(x).double()[None], (oh, ow), mode="bilinear", align_corners=True)[0].numpy()
        assert np.abs(out - ref).max() <= 1e-4 * np.abs(x).max(), name
        gin, _ = oracle_backward(g, *x.shape[1:])
        assert abs(float((out * g).sum()) - float((gin * x).sum())) <= 1e-9 * float(np.abs(out * g).sum()), name


def test_arguments_are_rejected_without_gpu(lib):
    d = _capi.VampResize2dDesc()
    one = torch.zeros(4)

    def fill(ih=4, iw=4, oh=8, ow=8, nseg=1, planes=1, src=one, dst=one):
        d.ih, d.iw, d.oh, d.ow, d.nseg = ih, iw, oh, ow, nseg
        for k in range(_capi.VAMP_RESIZE2D_MAX_SEGS):
            d.seg[k].src, d.seg[k].dst = (src.data_ptr() if src is not None else None), \
                (dst.data_ptr() if dst is not None else None)
            d.seg[k].planes = planes

    for fn in (lambda: lib.vamp_resize2d_forward(C.byref(d), None),
               lambda: lib.vamp_resize2d_backward(C.byref(d), None, 0, None)):
        for kw, message in ((dict(ih=0), b"sizes must be positive"), (dict(ow=-3), b"sizes must be positive"),
                            (dict(nseg=0), b"1 <= nseg <= 4"), (dict(nseg=5), b"1 <= nseg <= 4"),
                            (dict(planes=0), b"0 < planes"), (dict(planes=65536), b"0 < planes"),
                            (dict(src=None), b"NULL tensor"), (dict(dst=None), b"NULL tensor"),
                            (dict(ih=65536, iw=65536), b"plane too large"),
                            (dict(oh=46341, ow=46341), b"plane too large"),
                            (dict(ih=REFUSED[0], iw=REFUSED[1], oh=REFUSED[2], ow=REFUSED[3]), b"resize ratio outside")):
            fill(**kw)
            assert fn() == -1, kw
            assert message in lib.vamp_last_error(), (kw, lib.vamp_last_error())
    assert lib.vamp_resize2d_forward(None, None) == -1 and b"desc is NULL" in lib.vamp_last_error()
    assert lib.vamp_resize2d_backward(None, None, 0, None) == -1 and b"desc is NULL" in lib.vamp_last_error()


def test_cpu_tensors_raise():
    from vampire_amd import layers
    with pytest.raises(_capi.VampireHipError):
        layers.resize_bilinear2d(torch.zeros(1, 2, 3), (4, 6))
    with pytest.raises(_capi.VampireHipError):
        layers.resize_bilinear2d_pack([torch.zeros(1, 2, 3), torch.zeros(2, 2, 3)], (4, 6))


def test_supported_and_workspace_match_the_mirror(lib):
    shapes = [c[1:] for c in CASES.values()] + [REFUSED, (64, 176, 256, 704), (256, 256, 128, 128), (0, 4, 4, 4),
                                                 (4, 4, 4, 0), (65536, 65536, 4, 4), (1, 1, 4, 4), (1, 1, 5, 5),
                                                 (2, 2, 8, 8), (3, 2, 3, 9), (4, 4, 4000, 16), (4000, 4, 2, 16),
                                                 (4, 1000, 4, 4100), (4, 1000, 4, 4300), (4, 300, 4, 1300),
                                                 (4, 2000, 4, 100), (4, 257, 4, 1053), (4, 256, 4, 1049)]
    for iw in (1, 2, 3, 5, 16, 100, 255, 256, 257, 511, 513):
        for ow in sorted({1, iw, (iw + 1) // 2, int(iw / 2.1) + 1, 2 * iw, 4 * iw, int(4.1 * iw), int(4.1 * iw) + 1,
                          int(4.3 * iw) + 1, 5 * iw, 7 * iw, 8 * iw + 1}):
            shapes.append((3, iw, 7, ow))
    for s in shapes:
        assert lib.vamp_resize2d_supported(*s) == supported(*s), s
        assert lib.vamp_resize2d_workspace_bytes(*s) == 0, s           # run tables in registers and LDS: no scratch
    # what the header promises: every out / in <= 4.1 per axis, the identity, downsampling to out >= in / 2.1
    for n_in in list(range(1, 70)) + [175, 176, 255, 256, 257, 300, 512, 1000]:
        for n_out in {n_in, int(4.1 * n_in), 4 * n_in, 2 * n_in, int(n_in / 2.1) + 1, (n_in + 1) // 2}:
            assert lib.vamp_resize2d_supported(n_in, n_in, n_out, n_out) == 1, (n_in, n_out)
            assert lib.vamp_resize2d_supported(5, n_in, 3, n_out) == 1, (n_in, n_out)
    assert lib.vamp_resize2d_supported(*REFUSED) == 0


def _pairs():
    for n_in in range(1, 65):
        outs = set(range(1, int(4.1 * n_in) + 1)) if n_in > 1 else {1, 2, 3, 4}
        outs |= {(n_in + 1) // 2, n_in // 2, int(n_in / 2.1) + 1}
        for n_out in sorted(o for o in outs if o >= 1):
            yield n_in, n_out


def test_run_table_is_the_transpose_of_the_forward_taps():
    """Every in <= 64 with every out <= 4.1 in, and the 0.5x pairs, in float32: the outputs whose taps include a source
    index are the one contiguous run [F(i - 1), F(i + 1)) the kernel walks, the run fits the weight registers the
    launcher picks, and the run's weights are the forward's (each output's weights over the runs add up to l0 + l1)."""
    checked = 0
    for n_in, n_out in _pairs():
        i0, i1, l0, l1 = taps(n_in, n_out)
        assert np.all(np.diff(i0) >= 0) and i0.min() >= 0 and i1.max() <= n_in - 1
        idx = np.arange(n_in)
        begin, end = np.searchsorted(i0, idx - 1, "left"), np.searchsorted(i0, idx + 1, "left")
        o = np.arange(n_out)[:, None]
        run = (o >= begin[None]) & (o < end[None])                                  # [out, in]
        touch = (i0[:, None] == idx[None]) | (i1[:, None] == idx[None])
        assert np.array_equal(run, touch), (n_in, n_out)
        longest = int((end - begin).max())
        assert longest <= MAX_RUN and run_fits(n_in, n_out, MAX_RUN), (n_in, n_out, longest)
        for hits in (4, 10):
            assert not run_fits(n_in, n_out, hits) or longest <= hits, (n_in, n_out, hits, longest)
        table = np.where(i0[:, None] == idx[None], l0[:, None], np.float32(0)) \
            + np.where(i1[:, None] == idx[None], l1[:, None], np.float32(0))       # the kernel's weight expression
        assert table.dtype == np.float32 and np.all(table[~run] == 0)
        both = i0 == i1
        assert np.array_equal(table.astype(np.float64).sum(1)[~both], (l0.astype(np.float64) + l1)[~both])
        assert np.array_equal(table[both, i0[both]], (l0 + l1)[both])
        assert strip_fits(n_in, n_out)
        checked += 1
        if checked % 97 == 0 or n_in <= 3:              # the search the kernel runs, against the sorted lookup
            s = axis_scale(n_in, n_out)
            for v in range(-1, n_in + 2):
                assert first_at_least(s, n_out, v) == (int(np.searchsorted(i0, v, "left")) if v > 0 else 0)
    assert checked > 8000


def test_forward_fast_path_picks_the_tap_columns():
    """Mirror of the forward's choice for a thread's four neighbouring outputs (ow % 4 == 0), every iw < 80 with every
    ow <= 4.1 iw: where the last output's i1 lies at most two columns from the first output's i0, the thread loads the
    columns c0, c0 + 1, c0 + 2 (clamped to iw - 1) and every tap, i0 and i1 alike, finds its own column at its
    distance from c0 -- also the last output of a row, where i0 == i1 == iw - 1 == c0 + 2."""
    fast = at_the_end = 0
    for iw in range(1, 80):
        for ow in range(4, int(4.1 * iw) + 1, 4):
            i0, i1, _, _ = taps(iw, ow)
            for ox in range(0, ow, 4):
                c0 = int(i0[ox])
                if i1[ox + 3] - c0 > 2:
                    continue                     # the general path: a load per tap
                cols = [c0, min(c0 + 1, iw - 1), min(c0 + 2, iw - 1)]
                for v in range(ox, ox + 4):
                    d0, d1 = int(i0[v]) - c0, int(i1[v]) - c0
                    assert 0 <= d0 <= d1 <= 2 and cols[d0] == i0[v] and cols[d1] == i1[v], (iw, ow, v)
                    at_the_end += d0 == 2
                fast += 1
    assert fast > 10000 and at_the_end > 1000


# =============================================================================================== GPU tests
def _to(dev, *arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays]


def _check(name, y, gin, x, g):
    oh, ow = g.shape[1:]
    ref, bound = oracle_forward(x, oh, ow)
    e, r = worst(y.cpu().numpy(), ref, bound)
    print(f"{name}: forward max err {e:.3e}, {r:.3f} of the bound")
    rg, bg = oracle_backward(g, *x.shape[1:])
    eb, rb = worst(gin.cpu().numpy(), rg, bg)
    print(f"{name}: backward max err {eb:.3e}, {rb:.3f} of the bound")
    assert r <= 1 and rb <= 1, (name, r, rb)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_forward_backward_against_oracle(dev, name):
    from vampire_amd.layers import resize_bilinear2d
    x, g = case_inputs(name)
    xd, gd = _to(dev, x, g)
    xd.requires_grad_(True)
    y = resize_bilinear2d(xd, g.shape[1:])
    assert y.shape == gd.shape and y.dtype == torch.float32
    y.backward(gd)
    _check(name, y.detach(), xd.grad, x, g)


def _run_pack(dev, shapes, size, seed, skip=()):
    """Forward + backward of a pack; returns (inputs, outputs, upstream gradients, input gradients)."""
    from vampire_amd.layers import resize_bilinear2d_pack
    gen = torch.Generator().manual_seed(seed)
    xs = [torch.randn(s, generator=gen).to(dev).requires_grad_(True) for s in shapes]
    ys = resize_bilinear2d_pack(xs, size)
    gs = [torch.randn(y.shape, generator=gen).to(dev) for y in ys]
    keep = [k for k in range(len(ys)) if k not in skip]
    torch.autograd.backward([ys[k] for k in keep], [gs[k] for k in keep])
    return xs, ys, gs, [x.grad for x in xs]


@pytest.mark.gpu
def test_pack_equals_single_calls_bitwise(dev):
    """rgb (3), seg logits (18) and depth (1) of 2 images in one call each way against three calls."""
    from vampire_amd.layers import resize_bilinear2d
    shapes = [(2, 3, 4, 44), (2, 18, 4, 44), (2, 1, 4, 44)]
    xs, ys, gs, gins = _run_pack(dev, shapes, (16, 176), 1)
    for x, y, g, gin in zip(xs, ys, gs, gins):
        a = x.detach().clone().requires_grad_(True)
        b = resize_bilinear2d(a, (16, 176))
        b.backward(g)
        assert b.shape == y.shape == x.shape[:2] + (16, 176)
        assert torch.equal(b, y) and torch.equal(a.grad, gin)
        _check("pack", y.detach().flatten(0, 1), gin.flatten(0, 1), x.detach().flatten(0, 1).cpu().numpy(),
               g.flatten(0, 1).cpu().numpy())


@pytest.mark.gpu
def test_pack_of_four_around_the_plane_group(dev):
    shapes = [(GROUP - 1, 5, 7), (GROUP, 5, 7), (GROUP + 1, 5, 7), (2 * GROUP + 1, 5, 7)]
    xs, ys, gs, gins = _run_pack(dev, shapes, (20, 28), 2)
    for k, (x, y, g, gin) in enumerate(zip(xs, ys, gs, gins)):
        _check(f"segment {k}", y.detach(), gin, x.detach().cpu().numpy(), g.cpu().numpy())
    from vampire_amd.layers import resize_bilinear2d_pack
    with pytest.raises(ValueError):
        resize_bilinear2d_pack([x.detach() for x in xs] + [xs[0].detach()], (20, 28))
    with pytest.raises(ValueError):
        resize_bilinear2d_pack([xs[0].detach(), xs[1].detach()[:, :4]], (20, 28))


@pytest.mark.gpu
def test_pack_output_without_gradient_is_dropped(dev):
    """No gradient for the middle output: its input gets None (the segment is not launched), the others what they get
    when every output has one."""
    shapes = [(3, 5, 7), (4, 5, 7), (2, 5, 7)]
    _, _, _, full = _run_pack(dev, shapes, (19, 28), 3)
    _, _, _, part = _run_pack(dev, shapes, (19, 28), 3, skip=(1,))
    assert part[1] is None
    assert torch.equal(part[0], full[0]) and torch.equal(part[2], full[2])


@pytest.mark.gpu
def test_misaligned_and_sliced_views(dev):
    """Views that do not start on a 16-byte boundary and non-contiguous channel slices (inputs and upstream gradients):
    the `_aligned` copy makes them what the kernels take; results equal those of fresh contiguous tensors bit for bit."""
    from vampire_amd.layers import resize_bilinear2d
    gen = torch.Generator().manual_seed(4)
    flat = torch.randn(2 * 5 * 4 * 44 + 1, generator=gen).to(dev)
    gflat = torch.randn(2 * 3 * 16 * 176 + 3, generator=gen).to(dev)
    odd = flat[1:].view(2, 5, 4, 44)
    assert odd.data_ptr() % 16 != 0
    x = odd[:, 1:4]
    assert not x.is_contiguous()
    g = gflat[3:].view(2, 3, 16, 176)
    assert g.data_ptr() % 16 != 0
    a = x.detach().requires_grad_(True)
    y = resize_bilinear2d(a, (16, 176))
    y.backward(g)
    b = x.detach().clone().contiguous().requires_grad_(True)
    z = resize_bilinear2d(b, (16, 176))
    z.backward(g.clone())
    assert torch.equal(y, z) and torch.equal(a.grad, b.grad)
    _check("sliced view", y.detach().flatten(0, 1), a.grad.flatten(0, 1), x.flatten(0, 1).cpu().numpy(),
           g.flatten(0, 1).cpu().numpy())


def _desc(ih, iw, oh, ow, pairs):
    from vampire_amd.layers import _resize2d_desc
    return _resize2d_desc(ih, iw, oh, ow, pairs)


@pytest.mark.gpu
def test_c_abi_takes_misaligned_hi_res_tensors(dev):
    """Straight through the C ABI with the hi-resolution tensor 4 bytes off a 16-byte boundary (ow % 4 == 0): the
    launcher takes the scalar path; the results equal the 16-byte path's bit for bit."""
    from vampire_amd._tensors import _stream
    vamp = _capi.checked()
    p, ih, iw, oh, ow = CASES["x4 vector stores"]
    x, g = _to(dev, *case_inputs("x4 vector stores"))
    y, gin = torch.empty_like(g), torch.empty_like(x)
    vamp.vamp_resize2d_forward(_desc(ih, iw, oh, ow, [(x, y)]), _stream())
    vamp.vamp_resize2d_backward(_desc(ih, iw, oh, ow, [(g, gin)]), None, 0, _stream())
    y_off = torch.empty(g.numel() + 1, device=dev)[1:].view(g.shape)
    g_off = torch.empty(g.numel() + 1, device=dev)[1:].view(g.shape)
    g_off.copy_(g)
    gin2 = torch.empty_like(x)
    assert y_off.data_ptr() % 16 == 4 and g_off.data_ptr() % 16 == 4
    vamp.vamp_resize2d_forward(_desc(ih, iw, oh, ow, [(x, y_off)]), _stream())
    vamp.vamp_resize2d_backward(_desc(ih, iw, oh, ow, [(g_off, gin2)]), None, 0, _stream())
    assert torch.equal(y, y_off) and torch.equal(gin, gin2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["x4 vector stores", "x4 scalar tail 19x28", "down 9x13 -> 4x6", "out 1 along y",
                                  "column chunk + 1", "two bands + 1"])
def test_backward_is_repeatable_and_writes_every_pixel_once(dev, name):
    """Two backward runs agree bit for bit, and a NaN-prefilled grad_in has no NaN left: every source pixel is written,
    those nothing contributes to (9x13 -> 4x6 leaves whole rows and columns untouched) as 0."""
    from vampire_amd._tensors import _stream
    vamp = _capi.checked()
    p, ih, iw, oh, ow = CASES[name]
    x, g = case_inputs(name)
    (gd,) = _to(dev, g)
    runs = []
    for _ in range(2):
        gin = torch.full((p, ih, iw), float("nan"), device=dev)
        vamp.vamp_resize2d_backward(_desc(ih, iw, oh, ow, [(gd, gin)]), None, 0, _stream())
        assert not bool(torch.isnan(gin).any()), name
        runs.append(gin)
    assert torch.equal(runs[0], runs[1])
    ref, bound = oracle_backward(g, ih, iw)
    assert worst(runs[0].cpu().numpy(), ref, bound)[1] <= 1
    if name == "down 9x13 -> 4x6":
        assert bool((runs[0][:, 4] == 0).all()) and bool((runs[0][:, 7] == 0).all())


@pytest.mark.gpu
def test_refused_ratio_raises_and_the_backbone_keeps_aten(dev, monkeypatch):
    from vampire_amd import backbone
    from vampire_amd.layers import resize_bilinear2d
    x = torch.randn(2, *REFUSED[:2], device=dev)
    with pytest.raises(_capi.VampireHipError, match="resize ratio outside"):
        resize_bilinear2d(x, REFUSED[2:])
    monkeypatch.setattr(backbone.SWITCHES, "resize2d", True)
    assert backbone._resize2d_pack([x], REFUSED[2:]) is None              # refused: the caller's aten path runs
    assert backbone._resize2d_pack([x.half()], (8, 8)) is None            # not fp32
    assert backbone._resize2d_pack([x.cpu()], (8, 8)) is None             # not on the device
    got = backbone._resize2d_pack([x], (8, 8))
    assert got is not None and got[0].shape == (2, 8, 8)
    ref, bound = oracle_forward(x.cpu().numpy(), 8, 8)
    assert worst(got[0].cpu().numpy(), ref, bound)[1] <= 1
    monkeypatch.setattr(backbone.SWITCHES, "resize2d", False)
    assert backbone._resize2d_pack([x], (8, 8)) is None


@pytest.mark.gpu
def test_graph_capture_of_pack_forward_and_backward(dev):
    """One capture of the pack's forward + backward on one stream, replayed twice with fresh inputs: the replays equal
    the eager results bit for bit (the segment pointers travel in the launch arguments; nothing is read from host
    memory at replay)."""
    from vampire_amd.layers import resize_bilinear2d_pack
    shapes, size = [(2, 3, 4, 44), (2, 18, 4, 44), (2, 1, 4, 44)], (16, 176)
    gen = torch.Generator().manual_seed(5)
    gs = [torch.randn(s[:2] + size, generator=gen).to(dev) for s in shapes]

    def step():
        ys = resize_bilinear2d_pack(xs, size)
        return ys, torch.autograd.grad(ys, xs, gs)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        # the leaves first meet autograd on the capture stream: their gradient accumulators belong to it, and the
        # captured backward stays on the one stream
        xs = [torch.randn(sh, generator=gen).to(dev).requires_grad_(True) for sh in shapes]
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ys, gins = step()
    for seed in (6, 7):
        gen.manual_seed(seed)
        with torch.no_grad():
            for t in xs + gs:
                t.copy_(torch.randn(t.shape, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        eager_ys, eager_gins = step()
        assert all(torch.equal(a, b) for a, b in zip(ys, eager_ys))
        assert all(torch.equal(a, b) for a, b in zip(gins, eager_gins))


@pytest.mark.gpu
@pytest.mark.parametrize("det_step", [0.8, 0.05], ids=["16-cell grid", "256-cell grid"])
def test_backbone_with_the_switch_on_against_off(dev, monkeypatch, det_step):
    """The tiny BaseVAMPIRE2 of test_backbone_forward_backward with SWITCHES.resize2d on against off, same weights and
    inputs: the three resized camera maps agree within the forward bound (computed from the low-resolution maps the
    call received; both sides are blends of four roundings per term); on the 256-cell det grid, whose `voxel_output`
    ends in the 0.5x resize, the bev feature does so too within that resize's bound, on the 16-cell grid it has no
    resize and is bit-equal; every other output is bit-equal, parameter gradients agree within that test's tolerance."""
    from vampire_amd import backbone, synthetic
    from vampire_amd.backbone import BaseVAMPIRE2
    from vampire_amd.config import CFG_TINY as c
    kw = dict(x_bound_seg=list(c.x_bound_seg), y_bound_seg=list(c.y_bound_seg), z_bound_seg=list(c.z_bound_seg),
              x_bound_det=[-6.4, 6.4, det_step], y_bound_det=[-6.4, 6.4, det_step], z_bound_det=list(c.z_bound_det),
              d_bound=list(c.d_bound), final_dim=c.final_dim, downsample_factor=4, upsample_factor=4,
              mid_channels=4, output_channels=8, img_backbone_conf=dict(), img_neck_conf=dict(out_channels=[8] * 4),
              num_classes=5, density_mode="sdf", sdf_bias=-1.0, cat_pos=True, cat_seg=True)
    torch.manual_seed(0)
    mod = BaseVAMPIRE2(**kw).eval()
    with torch.no_grad():
        mod.density_conv.bias.fill_(-1.0)
    keys = list(mod.state_dict())
    half = isinstance(mod.voxel_output, torch.nn.Sequential)     # the 256-cell grid: 1x1 conv, then the 0.5x resize
    assert half == (det_step == 0.05)
    mod = mod.to(dev)
    B = 2
    s2e, K, ida = synthetic.camera_rig(c, B, src_hw=(64, 176), focal=60.0, centre=(88.0, 34.0), jitter=2.0, seed=4)
    s2e[:, :, :3, 3] *= 0.3
    mats = dict(sensor2ego_mats=s2e[:, None], intrin_mats=K[:, None], ida_mats=ida[:, None],
                sensor2sensor_mats=torch.eye(4).expand(B, 1, 6, 4, 4), bda_mat=synthetic.bda_matrix(B, rot_deg=8.0))
    mats = {k: v.to(dev) for k, v in mats.items()}
    imgs = torch.randn(B, 1, 6, 3, *c.final_dim).to(dev)
    seen = []
    pack = backbone._resize2d_pack
    monkeypatch.setattr(backbone, "_resize2d_pack", lambda ts, size: (seen.append([t.detach().clone() for t in ts]),
                                                                     pack(ts, size))[1])
    launches = []
    vamp = _capi.checked()
    monkeypatch.setattr(vamp, "vamp_resize2d_forward",
                        lambda d, s, _f=vamp.vamp_resize2d_forward: (launches.append(d.nseg), _f(d, s))[1])

    def run(on):
        monkeypatch.setattr(backbone.SWITCHES, "resize2d", on)
        mod.zero_grad(set_to_none=True)
        out = mod(imgs, mats)
        sum((o.float() ** 2).mean() for o in out[:8]).backward()
        return out, {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}

    off, g_off = run(False)
    assert launches == []
    del seen[:]
    on, g_on = run(True)
    # the three maps: one call, one launch; then the bev feature's 0.5x resize where the grid has one
    assert launches == ([3, 1] if half else [3]) and len(seen) == len(launches)
    assert list(mod.state_dict()) == keys
    checks = list(zip((1, 2, 3), seen[0])) + ([(0, seen[1][0])] if half else [])
    if half:
        assert seen[1][0].shape[-2:] == (256, 256) and on[0].shape[-2:] == (128, 128)
    for i, low in checks:
        ref, bound = oracle_forward(low.flatten(0, -3).cpu().numpy(), *on[i].shape[-2:])
        a, b = on[i].detach().flatten(0, -3).cpu().numpy(), off[i].detach().flatten(0, -3).cpu().numpy()
        e, r = worst(a, ref, bound)
        print(f"output {i}: switch on against the oracle: max err {e:.3e}, {r:.3f} of the bound")
        assert r <= 1, i
        # both sides are blends of four roundings per term, half the bound each
        assert np.all(np.abs(a.astype(np.float64) - b) <= bound), (i, float(np.abs(a - b).max()))
    for i in (4, 5, 6, 7) if half else (0, 4, 5, 6, 7):
        assert torch.equal(on[i], off[i]), i
    assert g_on.keys() == g_off.keys() and len(g_on) > 10
    for n in g_on:
        close(g_on[n], g_off[n], atol=1e-6, rtol=2e-3, scale="max", what="grad " + n)

