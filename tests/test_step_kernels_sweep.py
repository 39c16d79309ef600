"""The step-side kernels across the sizes that pick their code paths -- reg_loss.hip (the masked regression pack),
resize2d.hip (the 2-D bilinear resize) and param_update.hip (clip + AdamW + EMA) -- with the oracles, input builders,
error measures and bars of the kernels' own test modules (test_reg_loss, test_resize2d, test_param_update), none of them
restated or loosened: every case here is a shape, a placement or a sequence of steps those modules do not run.

reg_loss     single terms of 64, 65 and 129 workgroup slots (reg_finish_kernel's lane-strided walk takes one full trip,
             a second trip for one lane, a third), in fp32 and as bf16 / mse / clear / constant target; a mask set only
             in the slot the second trip reads; NaN / inf on the left-out side inside that slot; packs of T = 4, 5 and 7
             terms in which terms of 65 slots sit behind shorter ones (first[t] != 0) and on the second deal of a wave
             (t = wave + 4); grad_pred one element off its vector alignment through the C ABI (the forward took 16-byte
             loads, the backward takes element stores), fp32 and bf16.
resize2d     2 column chunks x 3 bands x 3 planes in one backward grid, on the 16-byte and the element path, as one
             segment and as a pack of 2 + 3 planes, also into a NaN-prefilled grad_in; runs of exactly 4, 10 and 16
             outputs in the 4, 10 and 16 instantiations (iw = 1) and runs of 14 and 15 in the 16 instantiation beyond
             two columns; the dispatch edges 4 | 10 | 16 from both sides; LDS strips of exactly 1088 columns (one chunk,
             a second chunk of 8, both chunks at the limit) and the refused neighbours; the forward's general path with
             17 planes (three plane groups, a last group of one) at VEC = 1 and VEC = 4; oh = 1 over two bands, 2 x 2.
param_update 1032 and 4102 parameter chunks (upd_finish_kernel's second trip; its unrolled block of four and a remainder)
             with an inf in a slot only the last trip reads; a parameter without a gradient on every step, one whose
             gradient appears at step 3 and one whose gradient vanishes after step 2 (the table is uploaded again; the
             one global step counter against torch's per-parameter one); ema_decay = 0; the loss scale's growth, its
             reset, static mode and the state_dict round trip; a NaN in the middle chunk of a tensor and an inf in the
             scalar tail of a misaligned gradient; beta1 = 0 without weight decay and clipping.

The CPU tests at the end mirror the host formulas that choose these paths, map every GPU case through them and fail
with the name of any listed regime that no case reaches, check the properties the cases are chosen for (longest runs,
strip spans, refusals), and compare the mirrors with vamp_reg_loss_workspace_bytes, vamp_param_update_workspace_bytes
and vamp_resize2d_supported over grids of descriptors that include sizes no GPU test could allocate.

Found here: no defect in a kernel.  ParamUpdate's docstring said a parameter without a gradient is skipped "as torch
skips it"; that holds for p, m and v of the skipped step, but the bias corrections of later steps use the one global
step counter where torch counts per parameter; test_update_gradient_appears_or_vanishes pins the
rule.

Measured on an MI355X: the 50 GPU tests of this file take 4.9 s in all; the slowest are the first reg_loss case (1.1 s
with the library's load and the first float64 oracle), the 1030-tensor bag (1.0 s, the first updater) and the first
resize case (0.7 s); no other case takes more than 0.35 s, the 4100-tensor bag 0.11 s.  Largest fraction of a bar:
reg_loss loss 0.055, grad_pred 0.056; resize2d forward 0.385, backward 0.298 of the bound; param_update 0.85 (exp_avg_sq
after a gradient vanished), p 0.59, EMA 0.50 -- where torch's fp32 error sets the bar the two errors are mostly the same
number, which is the fraction 0.5."""
import copy
import ctypes as C
import dataclasses
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import test_param_update as TP
import test_param_update_plan as TPP
import test_reg_loss as TL
import test_resize2d as TR
from vampire_amd import _capi, ops, optim
from vampire_amd import losses as L
from test_reg_loss import dev  # noqa: F401  (the module-scoped device fixture)

gpu = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
T, CH = ops.REG_TILE, optim.UPDATE_CHUNK
I31 = 0x7fffffff


def cdiv(a, b):
    return -(-a // b)


def align_up(v, a):
    return cdiv(v, a) * a


def _unreached(required, reached):
    return sorted(str(r) for r in set(required) - set(reached))


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# =====================================================================================================================
# reg_loss: mirrors, cases
# =====================================================================================================================
REG_WAVES, REG_LANES = 4, 64


def reg_tiles(n):
    return cdiv(n, T)


def reg_trips(n):
    """Trips of reg_finish_kernel's lane-strided walk over the term's slots."""
    return cdiv(reg_tiles(n), REG_LANES)


def reg_first(sizes):
    """first[t]: the term's first workgroup (slot); one more entry: the grid."""
    return [0] + list(itertools.accumulate(reg_tiles(n) for n in sizes))


def reg_owner(t):
    """(wave that finishes term t, which of that wave's deals)."""
    return t % REG_WAVES, t // REG_WAVES


def reg_workspace(sizes):
    if not (1 <= len(sizes) <= ops.REG_MAX_TERMS and all(1 <= n < 1 << 31 for n in sizes)):
        return 0
    blocks = reg_first(sizes)[-1]
    return align_up(blocks * 16, 256) + align_up(blocks * 8, 256)


@dataclasses.dataclass(frozen=True)
class RegCase:
    n: int
    kind: str = "smooth_l1"
    side: str = "both"
    dtype: torch.dtype = F32
    const: bool = False
    mask: str = "random"            # "random" | "last-tile": set only from element 64 T on


REG_SINGLE = {
    "slots64": RegCase(64 * T),
    "slots65": RegCase(64 * T + 1),
    "slots129": RegCase(128 * T + 5),
    "slots65-bf16-mse-clear-const": RegCase(64 * T + 1, "mse", "clear", BF16, True),
    "second-trip-alone": RegCase(64 * T + 1, side="set", mask="last-tile"),
}
REG_POISON_N = 64 * T + 7           # slot 64 holds seven elements
REG_POISON_SIDES = ("set", "clear")
# (n, kind, side, mask, dtype, constant target) per term
REG_PACKS = {
    4: [(3, "mse", "set", False, F32, True), (T - 1, "smooth_l1", "both", True, F32, False),
        (T + 1, "mse", "clear", True, BF16, False), (64 * T + 1, "smooth_l1", "both", True, F32, False)],
    5: [(T - 1, "smooth_l1", "clear", True, F32, True), (65 * T, "mse", "both", True, BF16, False),
        (3, "mse", "set", False, F32, False), (2 * T + 3, "smooth_l1", "set", True, BF16, True),
        (64 * T + 1, "smooth_l1", "both", True, F32, False)],
    7: [(3, "smooth_l1", "set", False, BF16, False), (T - 1, "mse", "both", True, F32, True),
        (T, "smooth_l1", "clear", True, F32, False), (1, "mse", "set", False, F32, True),
        (65 * T, "smooth_l1", "both", True, F32, False), (64 * T + 1, "mse", "clear", True, BF16, True),
        (64 * T + 1, "smooth_l1", "set", True, F32, False)],
}
REG_MISALIGNED = {"fp32": F32, "bf16": BF16}
REG_MISALIGNED_N = 2 * T + 3


@functools.lru_cache(maxsize=None)
def reg_single_inputs(name):
    c = REG_SINGLE[name]
    pred, target, mask = TL.make_case(c.n, seed=31 + list(REG_SINGLE).index(name), const=c.const)
    if c.mask == "last-tile":
        mask = torch.zeros(c.n, dtype=torch.bool)
        mask[64 * T:] = True
    return pred.to(c.dtype), target, mask


def reg_fraction(e_hip, e_torch):
    return e_hip / max(2 * e_torch, 1e-6)


@gpu
@pytest.mark.parametrize("name", list(REG_SINGLE))
def test_reg_single_terms(dev, name):
    """Loss and gradient against test_reg_loss.oracle at `within` and `one_ulp`, counts exact.  A bf16 pred is held
    through its fp32 twin, as test_bf16_pred_is_read_in_place does: the same loss bits, the twin's gradient rounded."""
    c = REG_SINGLE[name]
    pred, target, mask = reg_single_inputs(name)
    o_loss, o_grad, o_counts = TL.oracle(c.kind, c.side, pred, target, mask, upstream=TL.UP)
    loss, counts, grad = TL.run_hip(dev, pred.float(), target, mask, c.kind, c.side, upstream=TL.UP)
    t_loss, t_grad = TL.torch_host(c.kind, c.side, pred.float().to(dev), target, mask, upstream=TL.UP)
    e = (TL.rel(loss, o_loss), TL.rel(t_loss, o_loss), TL.gerr(grad, o_grad), TL.gerr(t_grad, o_grad))
    print(f"\n[reg:{name}] n {c.n}, slots {reg_tiles(c.n)}, finish trips {reg_trips(c.n)}, counts {tuple(counts.tolist())}, "
          f"fraction of the bar: loss {reg_fraction(e[0], e[1]):.3f}, grad {reg_fraction(e[2], e[3]):.3f}")
    assert tuple(counts.tolist()) == o_counts and counts.dtype == torch.int64
    TL.within(name + " loss", e[0], e[1])
    TL.within(name + " grad_pred", e[2], e[3])
    TL.one_ulp(name + " loss", loss, o_loss)
    TL.one_ulp(name + " grad_pred", grad, o_grad)
    assert bool((grad.cpu().numpy()[o_grad == 0] == 0).all())
    if c.dtype == BF16:
        a = TL.run_hip(dev, pred, target, mask, c.kind, c.side, upstream=TL.UP)
        assert a[2].dtype == BF16 and torch.equal(a[0], loss) and torch.equal(a[1], counts)
        assert torch.equal(a[2], grad.bfloat16())
    if c.mask == "last-tile":
        # one selected element, the only one of slot 64: the mean is its element loss, exactly
        assert o_counts == (1, 64 * T)
        le = TL.elem_torch(c.kind, pred[-1:], target[-1:])
        assert float(loss) == float(le[0]) and float(loss) > 0
        assert int((grad != 0).sum()) == 1 and float(grad[-1]) != 0


@gpu
@pytest.mark.parametrize("side", REG_POISON_SIDES)
def test_reg_poison_in_a_later_trip(dev, side):
    """NaN / +-inf in pred and target on the left-out side, inside slot 64 alone: bitwise the clean call."""
    n = REG_POISON_N
    pred, target, mask = TL.make_case(n, seed=41)
    mask[64 * T:] = torch.tensor([1, 0, 1, 0, 0, 1, 0], dtype=torch.bool)
    out = (~mask if side == "set" else mask).clone()
    out[:64 * T] = False
    assert 3 <= int(out.sum()) <= 4
    poison = torch.tensor([float("nan"), float("inf"), float("-inf"), float("nan")])[:int(out.sum())]
    for kind in TL.KINDS:
        clean = TL.run_hip(dev, pred, target, mask, kind, side, upstream=TL.UP)
        bad_p, bad_t = pred.clone(), target.clone()
        bad_p[out], bad_t[out] = poison, poison.flip(0)
        got = TL.run_hip(dev, bad_p, bad_t, mask, kind, side, upstream=TL.UP)
        assert bool(torch.isfinite(got[0])) and all(torch.equal(a, b) for a, b in zip(got, clean)), kind
        assert bool((got[2][out.to(dev)] == 0).all())
        o_loss, o_grad, o_counts = TL.oracle(kind, side, pred, target, mask, upstream=TL.UP)
        assert tuple(got[1].tolist()) == o_counts
        TL.one_ulp(f"poison {kind}/{side} loss", got[0], o_loss)
        TL.one_ulp(f"poison {kind}/{side} grad_pred", got[2], o_grad)


def reg_pack_terms(dev, spec, seed):
    terms = []
    for k, (n, kind, side, with_mask, dtype, const) in enumerate(spec):
        pred, target, mask = TL.make_case(n, seed=seed + k, with_mask=with_mask, const=const)
        x = pred.to(dev).to(dtype).requires_grad_(True)
        t = target.to(dev) if torch.is_tensor(target) else target
        terms.append(ops.RegTerm(x, t, None if mask is None else mask.to(dev), kind, side))
    return terms


@gpu
@pytest.mark.parametrize("nterms", list(REG_PACKS))
def test_reg_packs_are_bitwise_the_single_calls(dev, nterms):
    """As test_pack_is_bitwise_the_single_calls: losses, counts and gradients."""
    spec = REG_PACKS[nterms]
    terms = reg_pack_terms(dev, spec, 50 + nterms)
    w = torch.linspace(0.5, 2.25, nterms, device=dev)
    losses = ops.reg_losses(terms)
    assert losses.shape == (nterms,) and losses.counts.shape == (nterms, 2)
    (losses * w).sum().backward()
    pack_grads = [t.pred.grad.clone() for t in terms]
    first = reg_first([s[0] for s in spec])
    print(f"\n[reg:pack-T{nterms}] first {first}, trips {[reg_trips(s[0]) for s in spec]}, losses {losses.tolist()}")
    for k, t in enumerate(terms):
        t.pred.grad = None
        one = ops.reg_loss(*t)
        (one * w[k]).backward()
        assert torch.equal(one.detach(), losses[k].detach()), k
        assert torch.equal(one.counts, losses.counts[k]), k
        assert t.pred.grad.dtype == t.pred.dtype and torch.equal(t.pred.grad, pack_grads[k]), k
        assert int(one.counts.sum()) == t.pred.numel() and float(one) > 0


@gpu
@pytest.mark.parametrize("which", list(REG_MISALIGNED))
def test_reg_misaligned_grad_pred_through_the_c_abi(dev, which):
    """pred, target and mask aligned (the forward took group loads), grad_pred a slice one element into a buffer: the
    backward takes element accesses and gives the bits of the aligned call; the guards around the slice stay."""
    from vampire_amd._tensors import _stream
    dtype, n = REG_MISALIGNED[which], REG_MISALIGNED_N
    pred, target, mask = TL.make_case(n, seed=61)
    x, t, m = pred.to(dev).to(dtype), target.to(dev), mask.to(dev)
    (desc, nbytes, targets, masks), preds = L._reg_inputs([ops.RegTerm(x, t, m, "smooth_l1", "both")])
    ptrs = (L._ptr_array(preds), L._ptr_array(targets), L._ptr_array(masks))
    vamp = _capi.checked()
    losses = torch.empty(1, dtype=F32, device=dev)
    counts = torch.empty(1, 2, dtype=torch.int64, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    vamp.vamp_reg_loss_forward(desc, *ptrs, losses, counts, ws, nbytes, _stream())
    gl = torch.full((1,), TL.UP, dtype=F32, device=dev)
    aligned = torch.full((n,), 7.0, dtype=dtype, device=dev)
    buf = torch.full((n + 2,), 7.0, dtype=dtype, device=dev)
    off = buf[1:1 + n]
    ea = 8 if dtype == BF16 else 16
    assert all(p.data_ptr() % 16 == 0 for p in (preds[0], targets[0], masks[0], aligned)) and off.data_ptr() % ea != 0
    vamp.vamp_reg_loss_backward(desc, *ptrs, counts, gl, L._ptr_array([aligned]), _stream())
    vamp.vamp_reg_loss_backward(desc, *ptrs, counts, gl, L._ptr_array([off]), _stream())
    assert torch.equal(bits(aligned), bits(off))
    assert float(buf[0]) == 7.0 and float(buf[n + 1]) == 7.0
    want = TL.run_hip(dev, pred.to(dtype), target, mask, "smooth_l1", "both", upstream=TL.UP)
    assert torch.equal(want[0], losses[0]) and torch.equal(want[1], counts[0]) and torch.equal(bits(want[2]), bits(aligned))
    assert int((aligned.float() != 0).sum()) > n // 2


# =====================================================================================================================
# resize2d: mirrors (on top of test_resize2d's), cases
# =====================================================================================================================
RS_BAND, RS_COLS, RS_GROUP, RS_STRIP = TR.BAND, TR.COLS, TR.GROUP, TR.STRIP_MAX


def rs_mh(iw, ow):
    """The instantiation vamp_resize2d_backward picks."""
    return 4 if TR.run_fits(iw, ow, 4) else (10 if TR.run_fits(iw, ow, 10) else TR.MAX_RUN)


def rs_longest_run(n_in, n_out):
    """The most outputs whose taps include one source index (test_run_table_is_the_transpose_of_the_forward_taps)."""
    i0 = TR.taps(n_in, n_out)[0]
    idx = np.arange(n_in)
    return int((np.searchsorted(i0, idx + 1, "left") - np.searchsorted(i0, idx - 1, "left")).max())


def rs_spans(iw, ow):
    """Gradient columns of the LDS strip per chunk of source columns, as strip_fits rounds them."""
    s = TR.axis_scale(iw, ow)
    out = []
    for x0 in range(0, iw, RS_COLS):
        ob, oe = TR.first_at_least(s, ow, x0 - 1) & ~3, TR.first_at_least(s, ow, min(iw, x0 + RS_COLS))
        out.append((oe - ob + 3) // 4 * 4)
    return out


def rs_grid(p, ih, iw):
    return cdiv(iw, RS_COLS), cdiv(ih, RS_BAND), p


def rs_untouched_bands(ih, oh):
    """Bands of source rows whose range of gradient rows [F(y0 - 1), F(y1)) is empty."""
    s = TR.axis_scale(ih, oh)
    return [b for b in range(cdiv(ih, RS_BAND))
            if TR.first_at_least(s, oh, b * RS_BAND - 1) >= TR.first_at_least(s, oh, min(ih, (b + 1) * RS_BAND))]


def rs_forward_paths(iw, ow):
    """(VEC of contiguous tensors, the set of paths its threads take: "narrow" | "general")."""
    if ow % 4:
        return 1, {"general"}
    i0, i1, _, _ = TR.taps(iw, ow)
    return 4, {"narrow" if i1[ox + 3] - i0[ox] <= 2 else "general" for ox in range(0, ow, 4)}


def rs_plane_groups(p):
    g = cdiv(p, RS_GROUP)
    return g, p - (g - 1) * RS_GROUP


RS_CASES = {
    "decomposition-vector": (3, 17, 257, 35, 1028),
    "decomposition-scalar": (3, 17, 257, 35, 1027),
    "run4-of-MH4": (2, 3, 1, 5, 4),
    "run10-of-MH10": (2, 3, 1, 5, 10),
    "run16-of-MH16": (2, 3, 1, 5, 16),
    "run14-of-MH16": (2, 9, 40, 20, 261),
    "run15-of-MH16": (2, 3, 4, 5, 23),
    "edge-4-below-10": (2, 9, 9, 12, 12),
    "edge-10-above-4": (2, 9, 9, 13, 13),
    "edge-10-below-16": (2, 5, 21, 9, 81),
    "edge-16-above-10": (2, 5, 21, 9, 91),
    "strip-1088-vector": (1, 2, 256, 3, 1088),
    "strip-1088-and-8-scalar": (1, 2, 257, 3, 1089),
    "strip-1088-twice": (1, 2, 512, 3, 2172),
    "forward-general-VEC1-17-planes": (17, 9, 13, 4, 6),
    "forward-general-VEC4-17-planes": (17, 8, 8, 12, 12),
    "oh1-two-bands": (2, 9, 7, 1, 28),
    "out-2x2": (2, 7, 64, 2, 2),
}
RS_PACK = ("decomposition-vector", (2, 3))            # the case run as a pack of segments with these planes
RS_PREFILL = ("decomposition-vector", "decomposition-scalar", "oh1-two-bands")
RS_REFUSED = [(3, 1, 5, 17), (2, 256, 3, 1089), (2, 512, 3, 2173), (2, 512, 3, 2169), (2, 512, 3, 2170), (2, 512, 3, 2171)]


def rs_held(name, y, gin, x, g):
    """test_resize2d._check's comparison: (forward, backward) error over the bound, both at most 1."""
    ref, bound = TR.oracle_forward(x, *g.shape[1:])
    r = TR.worst(y.cpu().numpy(), ref, bound)[1]
    rg, bg = TR.oracle_backward(g, *x.shape[1:])
    rb = TR.worst(gin.cpu().numpy(), rg, bg)[1]
    assert r <= 1 and rb <= 1, (name, r, rb)
    return r, rb


def rs_describe(shape):
    p, ih, iw, oh, ow = shape
    return (f"MH {rs_mh(iw, ow)}, longest run {rs_longest_run(iw, ow)}, grid (chunks, bands, planes) {rs_grid(p, ih, iw)}, "
            f"spans {rs_spans(iw, ow)}, forward {rs_forward_paths(iw, ow)}, plane groups {rs_plane_groups(p)}")


@gpu
@pytest.mark.parametrize("name", list(RS_CASES))
def test_resize_paths(dev, name):
    from vampire_amd.layers import resize_bilinear2d
    shape = RS_CASES[name]
    x, g = TR.case_inputs(shape)
    xd, gd = TR._to(dev, x, g)
    xd.requires_grad_(True)
    y = resize_bilinear2d(xd, shape[3:])
    assert y.shape == gd.shape and y.dtype == F32
    y.backward(gd)
    r, rb = rs_held(name, y.detach(), xd.grad, x, g)
    print(f"\n[resize:{name}] {shape}: {rs_describe(shape)}; fraction of the bound: forward {r:.3f}, backward {rb:.3f}")


@gpu
def test_resize_decomposition_as_a_pack(dev):
    """The 2 x 3 x 3 grid once more with the planes in two segments (2 + 3): bitwise the single calls, which hold the
    bound."""
    from vampire_amd.layers import resize_bilinear2d, resize_bilinear2d_pack
    name, planes = RS_PACK
    _, ih, iw, oh, ow = RS_CASES[name]
    gen = torch.Generator().manual_seed(71)
    xs = [torch.randn(p, ih, iw, generator=gen).to(dev).requires_grad_(True) for p in planes]
    gs = [torch.randn(p, oh, ow, generator=gen).to(dev) for p in planes]
    ys = resize_bilinear2d_pack(xs, (oh, ow))
    torch.autograd.backward(ys, gs)
    for k, (x, y, g) in enumerate(zip(xs, ys, gs)):
        a = x.detach().clone().requires_grad_(True)
        b = resize_bilinear2d(a, (oh, ow))
        b.backward(g)
        assert torch.equal(b, y) and torch.equal(a.grad, x.grad), k
        rs_held(f"pack segment {k}", y.detach(), x.grad, x.detach().cpu().numpy(), g.cpu().numpy())


@gpu
@pytest.mark.parametrize("name", RS_PREFILL)
def test_resize_backward_writes_every_pixel_once(dev, name):
    """As test_backward_is_repeatable_and_writes_every_pixel_once: a NaN-prefilled grad_in has no NaN left, two runs
    agree bit for bit; a band no gradient row touches comes back as zeros."""
    from vampire_amd._tensors import _stream
    vamp = _capi.checked()
    p, ih, iw, oh, ow = RS_CASES[name]
    x, g = TR.case_inputs(RS_CASES[name])
    (gd,) = TR._to(dev, g)
    runs = []
    for _ in range(2):
        gin = torch.full((p, ih, iw), float("nan"), device=dev)
        vamp.vamp_resize2d_backward(TR._desc(ih, iw, oh, ow, [(gd, gin)]), None, 0, _stream())
        assert not bool(torch.isnan(gin).any()), name
        runs.append(gin)
    assert torch.equal(runs[0], runs[1])
    ref, bound = TR.oracle_backward(g, ih, iw)
    assert TR.worst(runs[0].cpu().numpy(), ref, bound)[1] <= 1
    for b in rs_untouched_bands(ih, oh):
        assert bool((runs[0][:, b * RS_BAND:(b + 1) * RS_BAND] == 0).all()), (name, b)
    if name == "oh1-two-bands":
        assert rs_untouched_bands(ih, oh) == [1] and bool((runs[0][:, 0] != 0).any()) and bool((runs[0][:, 1:] == 0).all())


@gpu
@pytest.mark.parametrize("shape", RS_REFUSED, ids=["x".join(map(str, s)) for s in RS_REFUSED])
def test_resize_refused_shapes_raise(dev, shape):
    """check_desc returns before any launch; the wrapper raises the library's message."""
    from vampire_amd.layers import resize_bilinear2d
    ih, iw, oh, ow = shape
    with pytest.raises(_capi.VampireHipError, match="resize ratio outside"):
        resize_bilinear2d(torch.zeros(1, ih, iw, device=dev), (oh, ow))


# =====================================================================================================================
# param_update: mirrors, cases, runners
# =====================================================================================================================
UPD_FINISH_BLOCK, UPD_UNROLL = 1024, 4
GROWTH = optim.GROWTH_INTERVAL
HYPER = dict(lr=1e-2, betas=TP.BETAS, eps=TP.EPS, weight_decay=0.01, max_norm=35.0, ema_decay=TP.DECAY,
             ema_updates=TP.UPDATES0)


def small_bag(n):
    return [1 + i % 7 for i in range(n)] + [CH + 5]


PU_FINISH = {"1030-tensors": (small_bag(1030), 1029), "4100-tensors": (small_bag(4100), 4098)}   # (sizes, tensor with the inf)
FOUR = [3, CH + 1, 70, 2 * CH + 3]
# tensor 1's gradient per step (True: present)
PU_PRESENCE = {"never": (False, False, False), "appears-at-step-3": (False, False, True, True),
               "vanishes-after-step-2": (True, True, False, False)}
# (tensor, element, value, the gradient is a slice one element into its buffer)
PU_OVERFLOW = {"nan-middle-chunk": (3, CH + 2 * 1024 + 5, float("nan"), False),
               "inf-unaligned-tail": (3, 2 * CH + 2, float("inf"), True)}


def upd_finish_trips(n_param):
    """(trips of lane 0 through upd_finish_kernel's walk, unrolled blocks of four among them, trips behind them)."""
    trips = cdiv(n_param, UPD_FINISH_BLOCK)
    return trips, trips // UPD_UNROLL, trips % UPD_UNROLL


def upd_plan(sizes):
    return optim.plan_update(sizes, [optim.KIND_PARAM] * len(sizes))


def upd_slot(sizes, tensor, element=0):
    """The parameter chunk (norm slot) that holds `element` of `tensor`."""
    pl = upd_plan(sizes)
    return int(np.nonzero((pl.tensor == tensor) & (pl.offset <= element) & (element < pl.offset + pl.length))[0][0])


def upd_valid(d):
    return (d.n_param_chunks >= 0 and d.n_buffer_chunks >= 0 and 1 <= d.n_param_chunks + d.n_buffer_chunks < 1 << 31
            and 0.0 <= d.beta1 < 1.0 and 0.0 <= d.beta2 < 1.0 and d.eps >= 0.0 and d.weight_decay >= 0.0
            and d.max_norm == d.max_norm and d.ema_decay < 1.0 and d.scale_mode in (0, 1, 2) and d.reserved == 0)


def upd_workspace(d):
    return align_up(max(d.n_param_chunks, 1) * 8, 256) if upd_valid(d) else 0


def bag_values(sizes, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen) * scale for n in sizes]


def bag_case(values, grads, **kw):
    """A test_param_update case (what run_torch and check_against_oracle take) of a Bag of `values` with the
    per-step gradient lists `grads`."""
    steps = len(grads)
    case = dict(net=TP.Bag([v.clone() for v in values]), grads=grads, bufs=[[] for _ in range(steps)], scales=[1.0] * steps,
                lrs=[HYPER["lr"]] * steps, skip=[False] * steps, weight_decay=HYPER["weight_decay"],
                max_norm=HYPER["max_norm"], steps=steps)
    case.update(kw)
    return case


class Stepper:
    """A Bag of device tensors under a ParamUpdate.  `packed`: the parameters are slices of one flat tensor (and the
    gradients of a step slices of another), so that thousands of them cost two copies."""

    def __init__(self, dev, values, packed=False, **kw):
        self.dev, self.sizes, self.packed = dev, [v.numel() for v in values], packed
        self.starts = [0] + list(itertools.accumulate(self.sizes))
        if packed:
            self.store = torch.cat(values).to(dev)
            vals = self.cut(self.store)
        else:
            vals = [v.to(dev) for v in values]
        self.bag = TP.Bag(vals)
        assert all(p.data_ptr() == t.data_ptr() for p, t in zip(self.bag.ps, vals))
        self.upd = optim.ParamUpdate(self.bag, **{**HYPER, **kw})
        offs = self.upd.plan.tensor_state_offset[:len(values)]
        self.index = torch.from_numpy(np.repeat(offs - np.asarray(self.starts[:-1]), self.sizes)
                                      + np.arange(self.starts[-1])).to(dev)

    def cut(self, flat):
        return [flat[a:b] for a, b in zip(self.starts[:-1], self.starts[1:])]

    def step(self, grads):
        """grads: a flat CPU tensor (packed), or a list of device tensors / None per parameter."""
        if torch.is_tensor(grads):
            grads = self.cut(grads.to(self.dev))
        for p, g in zip(self.bag.ps, grads):
            p.grad = g
        self.upd.step()
        return {k: v.item() for k, v in self.upd.stats.items()}

    def word(self, name, value=None):
        w = self.upd._scalars[optim._W[name]]
        if value is not None:
            w.fill_(value)
        return int(w)

    def state(self):
        """p, m, v, ema per tensor as fp32 CPU tensors (test_param_update.hip_state's shape)."""
        flat = self.flat_state()
        return {k: [t.clone() for t in self.cut(v[0])] for k, v in flat.items()}

    def flat_state(self):
        u = self.upd
        p = self.store if self.packed else torch.cat([q.detach() for q in self.bag.ps])
        out = {"p": p, "m": u.exp_avg[self.index], "v": u.exp_avg_sq[self.index]}
        if u.use_ema:
            out["ema"] = u.ema[self.index]
        return {k: [v.detach().cpu().clone()] for k, v in out.items()}


def same_bits(a, b, names=("p", "m", "v")):
    return all(torch.equal(bits(x), bits(y)) for n in names for x, y in zip(a[n], b[n]))


def bar_fractions(got, ref, e_torch):
    """Per name the largest error over the bar max(2 E_torch, 2^-22) of test_param_update.check_against_oracle; a
    reference tensor that is all zero must be met exactly."""
    out = {}
    for name in ref:
        for x, t, r in zip(got[name], e_torch[name], ref[name]):
            if float(r.abs().max()) == 0.0:
                assert float(x.abs().max()) == 0.0, name
                continue
            out[name] = max(out.get(name, 0.0), TP.rel_err(x, r) / max(2 * TP.rel_err(t, r), TP.FLOOR))
    return out


def held_to_the_bar(label, got, ref, e_torch):
    frac = bar_fractions(got, ref, e_torch)
    print(f"[update:{label}] fraction of the bar: " + ", ".join(f"{k} {v:.3f}" for k, v in frac.items()))
    assert all(v <= 1.0 for v in frac.values()), (label, frac)
    return frac


def checked_against_torch(label, case, ref, got):
    """check_against_oracle (the assertion), then the fractions of its bar for the record."""
    TP.check_against_oracle(case, ref, got, label)
    return held_to_the_bar(label, got, ref, TP.run_torch(case, F32, "cuda"))


def adamw_rule(values, grads, dtype, device, per_parameter_t, ema0=None, hyper=HYPER):
    """The update restated with torch operations in the order of torch's single-tensor AdamW: the norm over the
    gradients that are there, a parameter without one left as it is, the EMA line for every tensor.  The bias
    corrections take the number of steps taken so far (`per_parameter_t` False: ParamUpdate's one counter) or the
    number of gradients the parameter has had (True: torch.optim.AdamW's per-parameter step)."""
    to = lambda t: t.to(device=device, dtype=dtype).clone()
    (b1, b2), eps, wd, lr = hyper["betas"], hyper["eps"], hyper["weight_decay"], hyper["lr"]
    p = [to(v) for v in values]
    m, v = [torch.zeros_like(x) for x in p], [torch.zeros_like(x) for x in p]
    e = {str(i): to(x) for i, x in enumerate(ema0 or values)}
    own, updates = [0] * len(p), hyper["ema_updates"]
    for k, gs in enumerate(grads):
        gs = [None if g is None else to(g) for g in gs]
        norm = torch.sqrt(sum((g * g).sum() for g in gs if g is not None))
        coef = torch.clamp(hyper["max_norm"] / (norm + 1e-6), max=1.0)
        for i, g in enumerate(gs):
            if g is None:
                continue
            own[i] += 1
            t = own[i] if per_parameter_t else k + 1
            g = g * coef
            p[i].mul_(1 - lr * wd)
            m[i].lerp_(g, 1 - b1)
            v[i].mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (v[i].sqrt() / math.sqrt(1 - b2 ** t)).add_(eps)
            p[i].addcdiv_(m[i], denom, value=-(lr / (1 - b1 ** t)))
        updates += 1
        TP.ema_loop(e, {str(i): x for i, x in enumerate(p)}, updates, hyper["ema_decay"])
    out = {"p": p, "m": m, "v": v, "ema": list(e.values())}
    return {k: [t.double().cpu() for t in ts] for k, ts in out.items()}


@functools.lru_cache(maxsize=None)
def finish_inputs(name):
    """(values, three clean flat gradients of norm about 100, a fourth with an inf in the named tensor), CPU."""
    sizes, bad = PU_FINISH[name]
    values = bag_values(sizes, 80 + len(sizes))
    total = sum(sizes)
    gen = torch.Generator().manual_seed(81 + len(sizes))
    grads = [torch.randn(total, generator=gen) * (100.0 / math.sqrt(total)) for _ in range(4)]
    grads[3][sum(sizes[:bad])] = float("inf")
    return values, grads


@gpu
@pytest.mark.parametrize("name", list(PU_FINISH))
def test_update_finish_trips(dev, name):
    """Three clipped steps against float64 torch on one flat tensor of all the parameters (clip, AdamW and EMA are
    elementwise apart from the norm), then a step whose only inf lies in a slot the last trip reads."""
    sizes, bad = PU_FINISH[name]
    values, grads = finish_inputs(name)
    st = Stepper(dev, values, packed=True)
    n_param = st.upd.plan.n_param_chunks
    print(f"\n[update:finish-{name}] parameter chunks {n_param}, (trips, unrolled blocks, remainder) {upd_finish_trips(n_param)}, "
          f"slot of the inf {upd_slot(sizes, bad)}")
    for k in range(3):
        s = st.step(grads[k])
        tn = TP.norm_reference([grads[k]], 1.0)
        assert s["found_inf"] == 0 and s["step"] == k + 1 and 0.3 < s["clip_coef"] < 0.4
        TP.assert_within_one_ulp(s["total_norm"], tn)
        TP.assert_within_one_ulp(s["clip_coef"], HYPER["max_norm"] / (tn + 1e-6))
    flat = torch.cat(values)
    case = bag_case([flat], [[g] for g in grads[:3]])
    checked_against_torch(f"finish-{name}", case, TP.run_torch(case, torch.float64, "cpu"), st.flat_state())
    before = st.flat_state()
    s = st.step(grads[3])
    after = st.flat_state()
    assert s["found_inf"] == 1 and s["step"] == 3 and s["updates"] == TP.UPDATES0 + 4 and not math.isfinite(s["total_norm"])
    assert same_bits(before, after)
    assert not torch.equal(before["ema"][0], after["ema"][0])                  # the EMA ran on the unchanged weights
    ema = {"x": before["ema"][0].double()}
    TP.ema_loop(ema, {"x": before["p"][0].double()}, TP.UPDATES0 + 4, TP.DECAY)
    assert TP.rel_err(after["ema"][0], ema["x"]) <= TP.FLOOR


def four_inputs(steps, seed=90):
    values = bag_values(FOUR, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    total = sum(FOUR)
    grads = [[torch.randn(n, generator=gen) * (100.0 / math.sqrt(total)) for n in FOUR] for _ in range(steps)]
    return values, grads


def thin(grads, present):
    """Tensor 1's gradient taken out of the steps where it is not present."""
    return [[None if i == 1 and not there else g for i, g in enumerate(gs)] for gs, there in zip(grads, present)]


@gpu
def test_update_parameter_without_a_gradient(dev):
    """Tensor 1 never has a gradient: p, m, v keep their bits, its EMA (started away from p, so that the line shows)
    follows e d + (1 - d) p, the norm leaves it out; the other tensors are those of torch on a Bag without it."""
    present = PU_PRESENCE["never"]
    values, grads = four_inputs(len(present))
    st = Stepper(dev, values)
    ema0 = bag_values([FOUR[1]], 92)[0]
    st.upd._ema_views()[1].copy_(ema0.to(dev))
    start = st.state()
    ptrs = []
    for k, gs in enumerate(thin(grads, present)):
        s = st.step([None if g is None else g.to(dev) for g in gs])
        ptrs.append(st.upd._grad_ptrs[1])
        TP.assert_within_one_ulp(s["total_norm"], TP.norm_reference([g for g in gs if g is not None], 1.0))
        assert s["found_inf"] == 0 and s["step"] == k + 1
    got = st.state()
    assert ptrs == [0] * len(present)
    for name in ("p", "m", "v"):
        assert torch.equal(bits(got[name][1]), bits(start[name][1])), name
    assert float(got["m"][1].abs().max()) == 0.0 and float(got["v"][1].abs().max()) == 0.0
    ref, t32 = {"x": ema0.double()}, {"x": ema0.to(dev)}
    for k in range(len(present)):
        TP.ema_loop(ref, {"x": values[1].double()}, TP.UPDATES0 + k + 1, TP.DECAY)
        TP.ema_loop(t32, {"x": values[1].to(dev)}, TP.UPDATES0 + k + 1, TP.DECAY)
    held_to_the_bar("no-gradient ema", {"ema": [got["ema"][1]]}, {"ema": [ref["x"]]}, {"ema": [t32["x"].double().cpu()]})
    keep = [0, 2, 3]
    case = bag_case([values[i] for i in keep], [[gs[i] for i in keep] for gs in grads])
    checked_against_torch("no-gradient others", case, TP.run_torch(case, torch.float64, "cpu"),
                          {k: [v[i] for i in keep] for k, v in got.items()})


@gpu
@pytest.mark.parametrize("name", [k for k in PU_PRESENCE if k != "never"])
def test_update_gradient_appears_or_vanishes(dev, name):
    """The table is uploaded again when tensor 1's gradient comes or goes.  The results are those of the stated rule
    with the ONE step counter t; where the gradient first appears at step 3 they are not torch.optim.AdamW's, whose
    step is per parameter: torch moves the parameter by lr sign(g) there, the kernel by about 0.64 of that
    ((1 - beta1) / (1 - beta1^3) over sqrt((1 - beta2) / (1 - beta2^3))).  A gradient that vanishes gives torch's
    values: the skipped steps touch nothing, and no step follows them."""
    present = PU_PRESENCE[name]
    values, grads = four_inputs(len(present), seed=94)
    grads = thin(grads, present)
    st = Stepper(dev, values)
    ptrs = []
    for k, gs in enumerate(grads):
        s = st.step([None if g is None else g.to(dev) for g in gs])
        ptrs.append(st.upd._grad_ptrs[1])
        assert s["found_inf"] == 0 and s["step"] == k + 1
        TP.assert_within_one_ulp(s["total_norm"], TP.norm_reference([g for g in gs if g is not None], 1.0))
    assert [a != 0 for a in ptrs] == list(present)
    got = st.state()
    rule = adamw_rule(values, grads, torch.float64, "cpu", per_parameter_t=False)
    rule32 = adamw_rule(values, grads, F32, dev, per_parameter_t=False)
    held_to_the_bar(name, got, rule, rule32)
    torch64 = adamw_rule(values, grads, torch.float64, "cpu", per_parameter_t=True)
    torch32 = adamw_rule(values, grads, F32, dev, per_parameter_t=True)
    apart = TP.rel_err(got["p"][1], torch64["p"][1]) / max(2 * TP.rel_err(torch32["p"][1], torch64["p"][1]), TP.FLOOR)
    print(f"[update:{name}] tensor 1's p against per-parameter-step torch: {apart:.3g} bars")
    if name == "appears-at-step-3":
        assert apart > 100                                                      # the pinned difference is real
        # its first step, alone: (p - p') / lr is 0.64 sign(g) where torch gives sign(g)
        two = adamw_rule(values, grads[:3], torch.float64, "cpu", per_parameter_t=False)
        moved = (values[1].double() * (1 - HYPER["lr"] * HYPER["weight_decay"]) - two["p"][1]) / HYPER["lr"]
        ratio = (moved / torch.sign(grads[2][1].double())).median()
        assert abs(float(ratio) - 0.639) < 2e-3, float(ratio)
    else:
        held_to_the_bar(name + " against torch", got, torch64, torch32)


def run_net(case, dev, **kw):
    """test_param_update.run_hip with the updater's arguments open: (net, upd, per-step stats)."""
    net = copy.deepcopy(case["net"]).to(dev)
    args = dict(lr=case["lrs"][0], betas=case.get("betas", TP.BETAS), eps=TP.EPS, weight_decay=case["weight_decay"],
                max_norm=case["max_norm"], ema_decay=TP.DECAY, ema_updates=TP.UPDATES0)
    upd = optim.ParamUpdate(net, **{**args, **kw})
    stats = []
    for k in range(case["steps"]):
        with torch.no_grad():
            for (_, b), val in zip(TP.float_buffers(net), case["bufs"][k]):
                b.copy_(val)
        for p, g in zip(net.parameters(), case["grads"][k]):
            p.grad = g.to(dev)
        upd.step()
        stats.append({key: val.item() for key, val in upd.stats.items()})
    return net, upd, stats


def net_pmv(net, upd):
    offs = upd.plan.tensor_state_offset.tolist()
    params = list(net.parameters())
    return {"p": [p.detach().cpu() for p in params],
            "m": [upd.exp_avg[o:o + p.numel()].cpu() for p, o in zip(params, offs)],
            "v": [upd.exp_avg_sq[o:o + p.numel()].cpu() for p, o in zip(params, offs)]}


@gpu
def test_update_without_an_ema(dev):
    """ema_decay = 0 on the Net with float buffers: no EMA array, the buffer chunks are not launched, p, m, v are
    bitwise those of the run with an EMA."""
    case = TP.make_case(100.0, 0.01, steps=3, lrs=[1e-3] * 3)
    with_net, with_upd, _ = run_net(case, dev)
    net, upd, stats = run_net(case, dev, ema_decay=0)
    assert upd.ema.numel() == 0 and not upd.use_ema and upd.plan.n_buffer_chunks >= 3 and with_upd.ema.numel() > 0
    assert same_bits(net_pmv(net, upd), net_pmv(with_net, with_upd))
    assert [s["step"] for s in stats] == [1, 2, 3] and all(s["found_inf"] == 0 for s in stats)
    for (key, b), val in zip(TP.float_buffers(net), case["bufs"][-1]):
        assert torch.equal(bits(b.cpu()), bits(val)), key
    with pytest.raises(RuntimeError, match="without an EMA"):
        upd.ema_state_dict()
    for none in (None, -1.0):
        assert optim.ParamUpdate(copy.deepcopy(case["net"]).to(dev), lr=1e-3, ema_decay=none).ema.numel() == 0


def two_inputs():
    sizes = [3, CH + 1]
    values = bag_values(sizes, 96)
    gen = torch.Generator().manual_seed(97)
    grads = [[torch.randn(n, generator=gen) * 1000.0 for n in sizes] for _ in range(4)]
    bad = [g.clone() for g in grads[1]]
    bad[1][CH] = float("inf")
    return values, grads, bad


@gpu
def test_update_loss_scale_growth(dev):
    """The `growth` word set to the interval - 2 (no 2000-step loop): 65536, then 131072 with growth 0; an inf on the
    doubling step halves and resets instead; static mode keeps both; a state_dict taken at growth 1999 doubles on the
    fresh updater's next clean step and the two stay bitwise equal."""
    values, grads, bad = two_inputs()
    put = lambda gs: [g.to(dev) for g in gs]
    a = Stepper(dev, values, loss_scale="dynamic")
    assert a.word("growth", GROWTH - 2) == GROWTH - 2
    s = a.step(put(grads[0]))
    assert (s["scale"], a.word("growth"), s["found_inf"]) == (65536.0, GROWTH - 1, 0)
    saved = a.upd.state_dict()
    now = [p.detach().cpu().clone() for p in a.bag.ps]
    b, c = (Stepper(dev, now, loss_scale="dynamic", lr=1.0, ema_updates=0) for _ in range(2))
    for other in (b, c):
        other.upd.load_state_dict(saved)
        assert other.word("growth") == GROWTH - 1 and other.word("step") == 1
    s = c.step(put(bad))
    assert (s["scale"], c.word("growth"), s["found_inf"], s["step"]) == (32768.0, 0, 1, 1)
    for k, want in ((1, 131072.0), (2, 131072.0), (3, 131072.0)):
        sa, sb = a.step(put(grads[k])), b.step(put(grads[k]))
        assert sa == sb and sa["scale"] == want and sa["found_inf"] == 0 and sa["step"] == k + 1
        assert a.word("growth") == b.word("growth") == k - 1
        assert same_bits(a.state(), b.state(), ("p", "m", "v", "ema")) and torch.equal(a.upd._scalars, b.upd._scalars)
    d = Stepper(dev, values, loss_scale=1024.0)
    d.word("growth", GROWTH - 2)
    for k, gs in enumerate((grads[0], grads[1], bad)):
        s = d.step(put(gs))
        assert (s["scale"], d.word("growth"), s["found_inf"]) == (1024.0, GROWTH - 2, int(k == 2))


@gpu
@pytest.mark.parametrize("name", list(PU_OVERFLOW))
def test_update_overflow_positions(dev, name):
    """After one clean step: a non-finite value away from a tensor's first and last chunk start sets found_inf and
    leaves p, m, v bit for bit."""
    tensor, element, value, sliced = PU_OVERFLOW[name]
    values, grads = four_inputs(3, seed=98)
    st = Stepper(dev, values)
    assert st.step([g.to(dev) for g in grads[0]])["found_inf"] == 0
    before = st.state()
    gs = [g.to(dev) for g in grads[1]]
    if sliced:
        big = torch.zeros(FOUR[tensor] + 8, device=dev)
        big[1:1 + FOUR[tensor]] = gs[tensor]
        gs[tensor] = big[1:1 + FOUR[tensor]]
        assert gs[tensor].data_ptr() % 16 == 4
    gs[tensor][element] = value
    s = st.step(gs)
    assert s["found_inf"] == 1 and s["step"] == 1 and not math.isfinite(s["total_norm"])
    after = st.state()
    assert same_bits(before, after)
    assert all(not torch.equal(x, y) for x, y in zip(before["ema"], after["ema"]))
    s = st.step([g.to(dev) for g in grads[2]])
    assert s["found_inf"] == 0 and s["step"] == 2 and not same_bits(after, st.state())


@gpu
def test_update_hyper_parameter_edges(dev):
    """beta1 = 0 (bc1 = 1, m = m + (g - m) 1: g up to a rounding), no weight decay (the decay factor is exactly 1),
    max_norm None."""
    case = TP.make_case(100.0, 0.0, steps=3, lrs=[1e-3] * 3, max_norm=0.0)
    case["betas"] = (0.0, 0.999)
    net, upd, stats = run_net(case, dev, max_norm=None)
    for k, s in enumerate(stats):
        assert s["clip_coef"] == 1.0 and s["found_inf"] == 0
        TP.assert_within_one_ulp(s["total_norm"], TP.norm_reference(case["grads"][k], 1.0))
    got = TP.hip_state(net, upd)
    checked_against_torch("beta1=0 wd=0 no-clip", case, TP.run_torch(case, torch.float64, "cpu"), got)


# =====================================================================================================================
# CPU tests: what the cases reach, the stated properties of the inputs, the mirrors against the library
# =====================================================================================================================
def test_reg_cases_reach_every_regime():
    reached = set()
    for name, c in REG_SINGLE.items():
        pred, target, mask = reg_single_inputs(name)
        tiles, trips = reg_tiles(c.n), reg_trips(c.n)
        last = tiles - (trips - 1) * REG_LANES                                 # lanes with a slot in the last trip
        tag = f"{c.kind}-{c.side}-{str(c.dtype)[6:]}-{'const' if c.const else 'tensor'}"
        per_tile = [bool(mask[k * T:(k + 1) * T].any()) for k in range(tiles)]
        how = "selected-in-slot-64-alone" if per_tile == [False] * 64 + [True] else "random-mask"
        reached.add(f"single-trips{trips}-last-trip-lanes{last}-{tag}-{how}")
        assert pred.dtype == c.dtype and mask.numel() == c.n == pred.numel()
    for side in REG_POISON_SIDES:
        reached.add(f"poison-left-out-by-{side}-in-trip{reg_trips(REG_POISON_N)}-slot{reg_tiles(REG_POISON_N) - 1}")
    for nterms, spec in REG_PACKS.items():
        sizes = [s[0] for s in spec]
        first = reg_first(sizes)
        assert nterms == len(spec) and reg_workspace(sizes) > 0
        reached.add(f"pack-T{nterms}")
        for t, n in enumerate(sizes):
            wave, deal = reg_owner(t)
            if reg_trips(n) > 1:
                reached.add(f"T{nterms}-multi-trip-term-on-wave{wave}-deal{deal}-first{'0' if first[t] == 0 else '>0'}")
        reached |= {f"T{nterms}-{str(s[4])[6:]}-{s[1]}-{s[2]}-{'const' if s[5] else 'tensor'}" for s in spec}
    for which, dtype in REG_MISALIGNED.items():
        reached.add(f"misaligned-grad-{str(dtype)[6:]}-tiles{reg_tiles(REG_MISALIGNED_N)}-tail{REG_MISALIGNED_N % 4}")
    required = {
        "single-trips1-last-trip-lanes64-smooth_l1-both-float32-tensor-random-mask",
        "single-trips2-last-trip-lanes1-smooth_l1-both-float32-tensor-random-mask",
        "single-trips3-last-trip-lanes1-smooth_l1-both-float32-tensor-random-mask",
        "single-trips2-last-trip-lanes1-mse-clear-bfloat16-const-random-mask",
        "single-trips2-last-trip-lanes1-smooth_l1-set-float32-tensor-selected-in-slot-64-alone",
        "poison-left-out-by-set-in-trip2-slot64", "poison-left-out-by-clear-in-trip2-slot64",
        "pack-T4", "pack-T5", "pack-T7",
        "T4-multi-trip-term-on-wave3-deal0-first>0",
        "T5-multi-trip-term-on-wave1-deal0-first>0", "T5-multi-trip-term-on-wave0-deal1-first>0",
        "T7-multi-trip-term-on-wave0-deal1-first>0", "T7-multi-trip-term-on-wave1-deal1-first>0",
        "T7-multi-trip-term-on-wave2-deal1-first>0",
        "T4-bfloat16-mse-clear-tensor", "T5-bfloat16-mse-both-tensor", "T7-bfloat16-mse-clear-const",
        "misaligned-grad-float32-tiles3-tail3", "misaligned-grad-bfloat16-tiles3-tail3"}
    assert not _unreached(required, reached), f"reg_loss regimes no case reaches: {_unreached(required, reached)}"
    # what test_reg_loss runs: at most six slots and one trip; T = 1, 2, 8
    assert max(reg_trips(n) for n in TL.SIZES) == 1 and max(reg_tiles(n) for n in TL.SIZES) == 6
    assert (reg_trips(64 * T), reg_trips(64 * T + 1), reg_trips(128 * T + 5)) == (1, 2, 3)


def test_resize_cases_reach_every_regime():
    reached = set()
    for name, shape in RS_CASES.items():
        p, ih, iw, oh, ow = shape
        assert TR.supported(ih, iw, oh, ow) == 1, name
        mh, run = rs_mh(iw, ow), rs_longest_run(iw, ow)
        nchunk, nband, _ = rs_grid(p, ih, iw)
        vec = "vector" if ow % 4 == 0 else "scalar"
        spans = rs_spans(iw, ow)
        fvec, paths = rs_forward_paths(iw, ow)
        groups, last = rs_plane_groups(p)
        assert run <= mh and len(spans) == nchunk
        reached.add(f"MH{mh}-run{run}-iw{'1' if iw == 1 else '>1'}")
        if nchunk > 1 and nband > 1 and p > 1:
            reached.add(f"grid-{nchunk}x{nband}x{p}-MH{mh}-{vec}")
        if max(spans) == RS_STRIP:
            reached.add(f"strip-{'+'.join(map(str, spans))}-{vec}")
        if "general" in paths and groups > 1:
            reached.add(f"forward-general-VEC{fvec}-groups{groups}-last{last}")
        if rs_untouched_bands(ih, oh):
            reached.add(f"oh{oh}-bands{nband}-untouched{rs_untouched_bands(ih, oh)}")
        reached.add(f"out-{oh}x{ow}" if oh == ow == 2 else f"ratio-{iw}-to-{ow}-MH{mh}")
    name, planes = RS_PACK
    reached.add(f"pack-{'+'.join(map(str, planes))}-of-{rs_grid(sum(planes), *RS_CASES[name][1:3])}")
    for name in RS_PREFILL:
        p, ih, iw, oh, ow = RS_CASES[name]
        reached.add(f"prefill-{rs_grid(p, ih, iw)}-{'vector' if ow % 4 == 0 else 'scalar'}")
    for s in RS_REFUSED:
        assert TR.supported(*s) == 0, s
        reached.add(f"refused-{s[1]}-to-{s[3]}")
    required = ({"grid-2x3x3-MH10-vector", "grid-2x3x3-MH10-scalar", "MH4-run4-iw1", "MH10-run10-iw1", "MH16-run16-iw1",
                 "MH16-run14-iw>1", "MH16-run15-iw>1", "ratio-9-to-12-MH4", "ratio-9-to-13-MH10", "ratio-21-to-81-MH10",
                 "ratio-21-to-91-MH16", "strip-1088-vector", "strip-1088+8-scalar", "strip-1088+1088-vector",
                 "forward-general-VEC1-groups3-last1", "forward-general-VEC4-groups3-last1", "oh1-bands2-untouched[1]",
                 "out-2x2", "pack-2+3-of-(2, 3, 5)", "prefill-(2, 3, 3)-vector", "prefill-(2, 3, 3)-scalar",
                 "prefill-(1, 2, 2)-vector"}
                | {f"refused-{a}-to-{b}" for a, b in ((1, 17), (256, 1089), (512, 2173), (512, 2169), (512, 2170), (512, 2171))})
    assert not _unreached(required, reached), f"resize2d regimes no case reaches: {_unreached(required, reached)}"
    # what test_resize2d runs: never chunks, bands and planes together; no run beyond 10 outputs, so that the 16
    # instantiation never uses a weight register the 10 one lacks; no strip at the limit; at most 3 planes on the
    # forward's general path
    for p, ih, iw, oh, ow in TR.CASES.values():
        nchunk, nband, _ = rs_grid(p, ih, iw)
        assert not (nchunk > 1 and nband > 1 and p > 1) and max(rs_spans(iw, ow)) < RS_STRIP
        assert rs_longest_run(iw, ow) <= 10 and not (iw == 1 and ow > 1)
        assert "general" not in rs_forward_paths(iw, ow)[1] or p <= 3


def test_resize_inputs_have_the_stated_properties():
    runs = {name: rs_longest_run(*RS_CASES[name][2::2]) for name in RS_CASES}
    assert [runs[f"run{n}-of-MH{m}"] for n, m in ((4, 4), (10, 10), (16, 16), (14, 16), (15, 16))] == [4, 10, 16, 14, 15]
    assert [rs_mh(*RS_CASES[n][2::2]) for n in ("edge-4-below-10", "edge-10-above-4", "edge-10-below-16", "edge-16-above-10")] \
        == [4, 10, 10, 16]
    assert rs_spans(256, 1088) == [1088] and rs_spans(257, 1089) == [1088, 8] and rs_spans(512, 2172) == [1088, 1088]
    assert rs_spans(257, 1028) == rs_spans(257, 1027) and len(rs_spans(257, 1028)) == 2
    # 15 is the longest run any accepted width reaches for 1 < iw <= 64 (16 needs iw == 1), and 4 -> 23 reaches it
    longest = {}
    for iw in range(2, 65):
        for ow in range(1, 8 * iw + 2):
            if TR.supported(3, iw, 3, ow):
                longest[(iw, ow)] = rs_longest_run(iw, ow)
    assert max(longest.values()) == 15 and longest[(4, 23)] == 15 and len(longest) > 8000
    # support is not monotone in ow: 2172 is accepted over three refused widths
    assert [TR.supported(2, 512, 3, ow) for ow in (2168, 2169, 2170, 2171, 2172, 2173)] == [1, 0, 0, 0, 1, 0]
    assert [TR.supported(2, 256, 3, ow) for ow in (1088, 1089)] == [1, 0] and TR.supported(3, 1, 5, 17) == 0
    assert rs_forward_paths(13, 6) == (1, {"general"}) and "general" in rs_forward_paths(8, 12)[1]
    assert rs_plane_groups(17) == (3, 1) and rs_untouched_bands(9, 1) == [1] and rs_untouched_bands(17, 35) == []


def test_update_cases_reach_every_regime():
    reached = set()
    for name, (sizes, bad) in PU_FINISH.items():
        n_param = upd_plan(sizes).n_param_chunks
        trips, blocks, rest = upd_finish_trips(n_param)
        slot = upd_slot(sizes, bad)
        values, grads = finish_inputs(name)
        assert all(bool(torch.isfinite(g).all()) for g in grads[:3]) and int((~torch.isfinite(grads[3])).sum()) == 1
        assert math.isinf(float(grads[3][sum(sizes[:bad])]))
        reached.add(f"finish-trips{trips}-unrolled{blocks}-remainder{rest}")
        if slot // UPD_FINISH_BLOCK == trips - 1:
            reached.add(f"inf-read-in-trip{trips}-of-{trips}")
        if upd_slot(sizes, len(sizes) - 1, CH) == n_param - 1 and n_param - 1 >= UPD_FINISH_BLOCK:
            reached.add(f"two-chunk-tensor-behind-{len(sizes) - 1}-small")
    pl = upd_plan(FOUR)
    chunks_of = lambda t: int((pl.tensor == t).sum())
    for name, present in PU_PRESENCE.items():
        changes = [a != b for a, b in zip(present, present[1:])]
        kind = "never" if not any(present) else ("appears" if present[-1] else "vanishes")
        reached.add(f"gradient-{kind}-chunks{chunks_of(1)}-uploads{1 + sum(changes)}")
        if kind == "appears":
            reached.add(f"first-gradient-at-global-step{present.index(True) + 1}")
    for name, (tensor, element, value, sliced) in PU_OVERFLOW.items():
        chunk = element // CH
        where = "first" if chunk == 0 else ("last" if chunk == chunks_of(tensor) - 1 else "middle")
        tail = (FOUR[tensor] - element) <= FOUR[tensor] % 4 or (sliced and FOUR[tensor] - element <= 4)
        reached.add(f"{'nan' if value != value else 'inf'}-{where}-chunk-round{element % CH // 1024}-"
                    f"{'misaligned-tail' if sliced and tail else 'group'}")
    net = TP.Net(0)
    nbuf = sum(cdiv(v.numel(), CH) for _, v in TP.float_buffers(net))
    reached.add(f"no-ema-buffer-chunks{nbuf}")
    required = {"finish-trips2-unrolled0-remainder2", "finish-trips5-unrolled1-remainder1", "inf-read-in-trip2-of-2",
                "inf-read-in-trip5-of-5", "two-chunk-tensor-behind-1030-small", "two-chunk-tensor-behind-4100-small",
                "gradient-never-chunks2-uploads1", "gradient-appears-chunks2-uploads2", "gradient-vanishes-chunks2-uploads2",
                "first-gradient-at-global-step3", "nan-middle-chunk-round2-group", "inf-last-chunk-round0-misaligned-tail",
                "no-ema-buffer-chunks4"}
    assert not _unreached(required, reached), f"param_update regimes no case reaches: {_unreached(required, reached)}"
    # what test_param_update runs: well under one trip
    own = optim.plan_update([p.numel() for p in net.parameters()], [0] * len(list(net.parameters()))).n_param_chunks
    assert upd_finish_trips(own) == (1, 0, 1) and own < 100


def test_adamw_rule_with_a_step_per_parameter_is_torch():
    """The restatement the appear / vanish cases are held to, with per-parameter steps, against torch.optim.AdamW and
    clip_grad_norm_ themselves in float64 (a missing gradient: p.grad = None); with the one counter it differs exactly
    where a gradient first appears late."""
    for name, present in PU_PRESENCE.items():
        values, grads = four_inputs(len(present), seed=94)
        grads = thin(grads, present)
        mine = adamw_rule(values, grads, torch.float64, "cpu", per_parameter_t=True)
        one_t = adamw_rule(values, grads, torch.float64, "cpu", per_parameter_t=False)
        params = [torch.nn.Parameter(v.double().clone()) for v in values]
        opt = torch.optim.AdamW(params, lr=HYPER["lr"], betas=HYPER["betas"], eps=HYPER["eps"],
                                weight_decay=HYPER["weight_decay"], foreach=False)
        for gs in grads:
            for p, g in zip(params, gs):
                p.grad = None if g is None else g.double()
            torch.nn.utils.clip_grad_norm_(params, HYPER["max_norm"], foreach=False)
            opt.step()
        for i, p in enumerate(params):
            assert TP.rel_err(mine["p"][i], p.detach()) <= 1e-13, (name, i)
            if p in opt.state and "exp_avg" in opt.state[p]:
                assert TP.rel_err(mine["m"][i], opt.state[p]["exp_avg"]) <= 1e-13
                assert TP.rel_err(mine["v"][i], opt.state[p]["exp_avg_sq"]) <= 1e-13
            differs = TP.rel_err(one_t["p"][i], p.detach()) > 1e-6
            assert differs == (name == "appears-at-step-3" and i == 1), (name, i)


# ----------------------------------------------------------------------------------- the mirrors against the library
@pytest.fixture(scope="module")
def lib():
    from vampire_amd.build import build_library
    build_library(verbose=False)
    return _capi.load()


def test_reg_workspace_matches_the_mirror(lib):
    ns = [1, T - 1, T, T + 1, 64 * T, 64 * T + 1, 128 * T + 5, 1 << 24, I31 - T, I31 - 1, I31, 0, 1 << 31]
    count = 0
    for nterms in range(0, 10):
        for combo in itertools.islice(itertools.product(ns, repeat=2), 0, None, 3):
            sizes = [combo[k % 2] if k % 3 else ns[(k + nterms) % len(ns)] for k in range(nterms)]
            d = _capi.VampRegLossDesc()
            d.T = nterms
            for k, n in enumerate(sizes[:ops.REG_MAX_TERMS]):
                d.terms[k].n = n
            want = reg_workspace(sizes) if nterms <= ops.REG_MAX_TERMS else 0
            assert lib.vamp_reg_loss_workspace_bytes(C.byref(d)) == want, sizes
            count += want > 0
    assert count > 100
    assert reg_workspace([I31] * 8) == align_up(8 * (1 << 19) * 16, 256) + align_up(8 * (1 << 19) * 8, 256)
    for spec in REG_PACKS.values():
        assert reg_first([s[0] for s in spec])[-1] == sum(reg_tiles(s[0]) for s in spec)


def test_update_workspace_matches_the_mirror(lib):
    count = 0
    for n_param, n_buf, beta1, ema, mode in itertools.product(
            (0, 1, 80, 1023, 1024, 1025, 4096, 4102, 12903, 10 ** 6, (1 << 31) - 2, (1 << 31) - 1, -1), (0, 1, 4523, 1 << 30),
            (0.0, 0.9, 1.0), (-1.0, 0.0, 0.999, 1.0), (0, 2, 3)):
        d = TPP._desc(n_param_chunks=n_param, n_buffer_chunks=n_buf, beta1=beta1, ema_decay=ema, scale_mode=mode)
        assert lib.vamp_param_update_workspace_bytes(C.byref(d)) == upd_workspace(d), (n_param, n_buf, beta1, ema, mode)
        count += upd_valid(d)
    assert count > 100 and upd_workspace(TPP._desc(n_param_chunks=10 ** 6)) == 8 * 10 ** 6
    assert [upd_finish_trips(n) for n in (1, 1024, 1025, 4096, 4097, 10 ** 6)] == [(1, 0, 1), (1, 0, 1), (2, 0, 2), (4, 1, 0),
                                                                                  (5, 1, 1), (977, 244, 1)]
    for sizes, _ in PU_FINISH.values():
        pl = upd_plan(sizes)
        assert pl.n_param_chunks == len(sizes) + 1 == sum(cdiv(n, CH) for n in sizes)


def test_resize_supported_matches_the_mirror(lib):
    count = 0
    for iw in (1, 2, 3, 4, 21, 40, 255, 256, 257, 511, 512, 513, 1000, 1024, 2047, 2048, 2049, 4095, 4096):
        outs = {1, 2, iw, 2 * iw, 4 * iw, int(4.1 * iw), int(4.2 * iw), int(4.25 * iw), 5 * iw, 16, 17, (iw + 1) // 2}
        outs |= {int(4.25 * iw) + k for k in range(-6, 7)} | {4 * iw + k for k in range(-3, 4)}
        for ow in sorted(o for o in outs if o >= 1):
            for ih, oh in ((3, 5), (1, 1)):
                assert lib.vamp_resize2d_supported(ih, iw, oh, ow) == TR.supported(ih, iw, oh, ow), (ih, iw, oh, ow)
                count += 1
    assert count > 1000
    for name, (p, ih, iw, oh, ow) in RS_CASES.items():
        assert lib.vamp_resize2d_supported(ih, iw, oh, ow) == 1, name
    for s in RS_REFUSED:
        assert lib.vamp_resize2d_supported(*s) == 0, s
