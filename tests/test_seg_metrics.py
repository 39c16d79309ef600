"""Lidar-segmentation and occupancy mIoU (vampire_amd.metrics over the HIP confusion-matrix and lidar-seg
prediction kernels).  The reference's metric code (base_exp.py:370-382, :634-663, :851-910 with
torchmetrics 0.11's multiclass JaccardIndex) is restated in torch / numpy below."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, metrics, ops                  # noqa: E402
from vampire_amd import multitask as M                       # noqa: E402
from vampire_amd.build import build_library                  # noqa: E402
from vampire_amd.config import CFG_TINY                      # noqa: E402


# ----------------------------------------------------------------------------- the reference, restated
def ref_confmat(logits_or_preds, target, mask=None, window=None, Kc=None, ignore_index=None):
    """torchmetrics' multiclass confusion matrix (confmat[target, pred]) of the boolean-indexed argmax,
    and the number of targets out of [0, Kc) (torchmetrics raises on them).  CPU."""
    x, t = logits_or_preds.cpu(), target.cpu().long()
    if mask is not None:
        x, t = x[mask.cpu()], t[mask.cpu()]
    if x.is_floating_point():
        lo, hi = window or (0, x.shape[-1])
        p = x.reshape(-1, x.shape[-1])[:, lo:hi].float().argmax(1) + lo
    else:
        p = x.reshape(-1).long()
    t = t.reshape(-1)
    if ignore_index is not None:
        keep = t != ignore_index
        p, t = p[keep], t[keep]
    ok = (t >= 0) & (t < Kc) & (p >= 0) & (p < Kc)
    cm = torch.bincount(t[ok] * Kc + p[ok], minlength=Kc * Kc).reshape(Kc, Kc)
    return cm, int((~ok).sum())


def ref_iou(cm):
    """torchmetrics 0.11 `_jaccard_index_reduce(average='none')`: diag / (rows + cols - diag), a zero
    denominator counted as 1 (`_safe_divide`)."""
    cm = cm.double()
    num = cm.diagonal()
    den = cm.sum(0) + cm.sum(1) - num
    den[den == 0] = 1
    return num / den


def ref_lidarseg_labels(pts_logits, ref_index, num_ref, lo, hi):
    """base_exp.py:835-838: zeros + sequential CPU index_add_, argmax over [lo, hi) + lo."""
    ref = torch.zeros(num_ref, pts_logits.shape[1])
    ref.index_add_(0, ref_index.cpu(), pts_logits.cpu().float())
    return ref[:, lo:hi].argmax(1) + lo


# ----------------------------------------------------------------------------- CPU: compute / epoch_end
def test_compute_formula_zero_union_and_empty():
    j = metrics.JaccardIndex(4, device="cpu")
    assert torch.equal(j.compute(), torch.zeros(4, dtype=torch.float64))      # empty state
    cm = torch.tensor([[5, 1, 0, 0], [2, 3, 0, 0], [0, 4, 0, 0], [0, 0, 0, 0]])
    j.confmat.copy_(cm)
    got = j.compute()
    assert got.dtype == torch.float64
    exp = [5 / (6 + 7 - 5), 3 / (5 + 8 - 3), 0.0, 0.0]            # class 2: no hit, class 3: union 0
    assert got.tolist() == pytest.approx(exp, rel=0, abs=0)
    assert torch.equal(got, ref_iou(cm))
    j.invalid.fill_(2)
    with pytest.raises(ValueError):
        j.compute()
    j.reset()
    assert int(j.invalid) == 0 and int(j.confmat.sum()) == 0


def test_epoch_end_drops_ignore_and_free():
    names = ["other", "a", "b", "c", "free"]
    ev = metrics.SegEvaluator(5, class_names=names, device="cpu")
    # lidar: 4 classes, iou = [x, 1, 0.5, 0] -> mIoU over [1:]; class 0 (ignored) has a value of its own
    ev.val_iou.confmat.copy_(torch.tensor([[7, 0, 0, 0], [0, 2, 0, 0], [0, 0, 1, 1], [0, 0, 0, 0]]))
    # occupancy: 5 classes, the last ("free") perfect and left out of the mean
    ev.occ_val_iou.confmat.copy_(torch.diag(torch.tensor([1, 1, 0, 0, 9])) + torch.tensor(
        [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]))
    out = ev.epoch_end("val")
    assert out["val/mIoU"] == pytest.approx((1 + 0.5 + 0) / 3, abs=0)
    assert out["val/occ_mIoU"] == pytest.approx((1 + 0.5 + 0 + 0) / 4, abs=0)
    assert [k for k in out if k.startswith("val/iou/")] == ["val/iou/a", "val/iou/b", "val/iou/c"]
    assert len([k for k in out if k.startswith("val/occ_iou/")]) == 4 and "val/occ_iou/free" not in out
    assert ev.best_miou == out["val/mIoU"] and ev.best_occ_miou == out["val/occ_mIoU"]
    assert int(ev.val_iou.confmat.sum()) == 0 and int(ev.occ_val_iou.confmat.sum()) == 0     # reset
    tr = ev.epoch_end("train")                           # empty train metrics: zeros, best untouched
    assert tr["train/mIoU"] == 0.0 and ev.best_miou == out["val/mIoU"]


def test_class_names_are_the_references():
    assert len(metrics.CLASS_NAMES) == 18 and metrics.CLASS_NAMES[0] == "other" and metrics.CLASS_NAMES[-1] == "free"
    ev = metrics.SegEvaluator(device="cpu")
    assert len(ev.lidar_names) == 16 and ev.val_iou.num_classes == 17 and ev.val_iou.ignore_index == 0
    assert ev.occ_val_iou.num_classes == 18 and ev.occ_val_iou.ignore_index is None


# ----------------------------------------------------------------------------- CPU: the C ABI
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(**kw):
    d = dict(B=1, S=10, K=18, layout=_capi.VAMP_SEG_ROWS, pred_dtype=_capi.VAMP_F32, target_dtype=_capi.VAMP_I64,
             Kc=18, lo=0, hi=18, ignore_index=0, use_ignore=0, reserved=0)
    d.update(kw)
    return _capi.VampConfDesc(**d)


def test_confusion_descriptor_size():
    assert C.sizeof(_capi.VampConfDesc) == 2 * 8 + 10 * 4


@pytest.mark.parametrize("bad", [dict(Kc=0), dict(Kc=33), dict(lo=5, hi=5), dict(lo=-1), dict(hi=19),
                                 dict(Kc=17, hi=18), dict(pred_dtype=7), dict(target_dtype=_capi.VAMP_F32),
                                 dict(layout=2), dict(B=1 << 16, S=1 << 15), dict(S=-1),
                                 dict(pred_dtype=_capi.VAMP_I64, K=18)])
def test_confusion_rejects_bad_arguments_without_gpu(lib, bad):
    d = _desc(**bad)
    assert lib.vamp_confusion_workspace_bytes(C.byref(d)) == 0
    assert lib.vamp_confusion_update(C.byref(d), None, None, None, None, None, None, 0, None) == -1
    assert b"requirement failed" in lib.vamp_last_error()


def test_confusion_rejects_null_pointers_without_gpu(lib):
    d = _desc()
    assert lib.vamp_confusion_workspace_bytes(C.byref(d)) > 0
    assert lib.vamp_confusion_update(None, None, None, None, None, None, None, 0, None) == -1
    assert lib.vamp_confusion_update(C.byref(d), None, None, None, None, None, None, 0, None) == -1
    assert b"confmat" in lib.vamp_last_error()


@pytest.mark.parametrize("args", [(10, 18, _capi.VAMP_F32, 3, 3, 5), (10, 18, _capi.VAMP_F32, 0, 19, 5),
                                  (10, 18, _capi.VAMP_I64, 1, 17, 5), (-1, 18, _capi.VAMP_F32, 1, 17, 5),
                                  (10, 100, _capi.VAMP_F32, 0, 100, 5), (10, 18, _capi.VAMP_F32, 1, 17, -2)])
def test_lidarseg_rejects_bad_arguments_without_gpu(lib, args):
    P, K, dt, lo, hi, R = args
    rc = lib.vamp_lidarseg_predict(P, K, dt, lo, hi, None, None, R, None, None, None, 0, None)
    assert rc == -1 and b"requirement failed" in lib.vamp_last_error()


def test_lidarseg_rejects_null_output_without_gpu(lib):
    assert lib.vamp_lidarseg_workspace_bytes(-1, 3) == 0
    assert lib.vamp_lidarseg_predict(10, 18, _capi.VAMP_F32, 1, 17, None, None, 5, None, None, None, 0, None) == -1
    assert b"invalid is NULL" in lib.vamp_last_error()


def test_operators_refuse_cpu_tensors():
    cm, inv = torch.zeros(4, 4, dtype=torch.int64), torch.zeros((), dtype=torch.int64)
    with pytest.raises(_capi.VampireHipError):
        ops.confusion_update(cm, inv, torch.randn(10, 4), torch.zeros(10, dtype=torch.int64))
    with pytest.raises(_capi.VampireHipError):
        ops.lidarseg_predict(torch.randn(10, 4), torch.zeros(10, dtype=torch.int64), 5, (1, 3))
    with pytest.raises(_capi.VampireHipError):
        metrics.JaccardIndex(4, device="cpu").update(torch.randn(10, 4), torch.zeros(10, dtype=torch.int64))


# ----------------------------------------------------------------------------- CPU: sync over gloo
def _sync_worker(rank, world, port, out):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    j = metrics.JaccardIndex(3, device="cpu")
    j.confmat.copy_(torch.arange(9).reshape(3, 3) * (rank + 1))
    j.invalid.fill_(rank + 5)
    j.sync()
    out[rank] = (j.confmat.numpy().copy(), int(j.invalid))
    dist.destroy_process_group()


def test_sync_sums_state_over_two_gloo_ranks():
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_sync_worker, args=(2, port, out), nprocs=2, join=True)
    for r in range(2):
        cm, inv = out[r]
        assert np.array_equal(cm, np.arange(9).reshape(3, 3) * 3) and inv == 11


def test_sync_without_process_group_is_a_noop():
    j = metrics.JaccardIndex(3, device="cpu")
    j.confmat.fill_(2)
    j.sync()
    assert int(j.confmat.sum()) == 18


# ----------------------------------------------------------------------------- CPU: the validation batch
def test_synthetic_val_batch_layout():
    cfg = CFG_TINY
    b = M.synthetic_val_batch(cfg, 2, seed=3, num_points=60, num_ref=70)
    assert len(b) == 15
    imgs, mats, ts, metas, boxes, labels, pts, pts_lab, ref_lab, ref_idx, tokens, occ, dens, ml, mc = b
    assert imgs.shape == (2, 1, cfg.num_cams, 3) + tuple(cfg.final_dim) and set(mats) == {
        "sensor2ego_mats", "intrin_mats", "ida_mats", "sensor2sensor_mats", "bda_mat"}
    assert ts.shape == (2, 1) and len(metas) == 2 and len(boxes) == 2 and boxes[0].shape[1] == 9
    assert len(pts) == 2 and pts[0].shape == (60, 3) and pts_lab[0].shape == (60,) and pts_lab[0].dtype == torch.int64
    assert ref_lab[0].shape == (70,) and ref_lab[0].dtype == torch.int64
    assert ref_idx[0].shape == (60,) and ref_idx[0].dtype == torch.int64
    assert 0 <= int(ref_idx[0].min()) and int(ref_idx[0].max()) < 70
    used = torch.unique(ref_idx[0])
    assert len(used) < 60 and len(used) < 70            # repeats, and reference points no point maps to
    assert isinstance(tokens[0], str)
    assert occ.shape == (2, 200, 200, 16) and occ.dtype == torch.int64 and dens.shape == occ.shape
    assert ml.dtype == torch.bool and mc.dtype == torch.bool and mc.shape == occ.shape


# ============================================================================= GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _run(x, t, mask=None, window=None, ignore=None, Kc=None, state=None):
    cm, inv = state if state is not None else (torch.zeros(Kc, Kc, dtype=torch.int64, device=t.device),
                                               torch.zeros((), dtype=torch.int64, device=t.device))
    ops.confusion_update(cm, inv, x, t, mask, class_window=window, ignore_index=ignore)
    return cm, inv


def _check(x, t, mask=None, window=None, ignore=None, Kc=None):
    Kc = Kc or x.shape[-1]
    cm, inv = _run(x, t, mask, window, ignore, Kc)
    rcm, rinv = ref_confmat(x, t, mask, window, Kc, ignore)
    assert torch.equal(cm.cpu(), rcm), (cm.cpu() - rcm).abs().max()
    assert int(inv) == rinv
    return rcm


def _occ_view(B, K, dev, dtype=torch.float32, g=None, shape=(200, 200, 16)):
    """occ_logits as the backbone returns them: permute(0, 2, 3, 4, 1) of a contiguous [B, K, X, Y, Z]."""
    vol = torch.randn((B, K) + shape, generator=g).to(dtype)
    return vol.to(dev).permute(0, 2, 3, 4, 1)


@gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_confusion_occupancy_view(dev, dtype):
    g = torch.Generator().manual_seed(1)
    K = 18
    x = _occ_view(2, K, dev, dtype, g)
    assert not x.is_contiguous()
    t = torch.randint(0, K, (2, 200, 200, 16), generator=g).to(dev)
    m = (torch.rand(2, 200, 200, 16, generator=g) < 0.5).to(dev)
    cm = _check(x, t, m)
    assert int(cm.sum()) == int(m.sum())
    _check(x, t)                                                  # without a mask


@gpu
def test_confusion_ties_nans_targets_and_ignore(dev):
    g = torch.Generator().manual_seed(2)
    K = 18
    vol = (torch.randn(2, K, 40, 40, 16, generator=g) * 2).round() / 2              # ties are common
    vol[torch.rand(vol.shape, generator=g) < 0.02] = float("nan")
    vol[0, :, 0, 0, 0] = float("nan")                                               # all-NaN element
    vol[0, :, 0, 0, 1] = float("-inf")                                              # all -inf element
    x = vol.to(dev).permute(0, 2, 3, 4, 1)
    t = torch.randint(0, K, (2, 40, 40, 16), generator=g)
    m = torch.rand(2, 40, 40, 16, generator=g) < 0.7
    for tt in (t, t.to(torch.uint8), t.to(torch.int32)):
        _check(x, tt.to(dev), m.to(dev))
        _check(x, tt.to(dev), m.to(dev), ignore=3)
    _check(x.to(torch.bfloat16), t.to(dev), m.to(dev))


@gpu
@pytest.mark.parametrize("n", [1, 7, 257, 35011])
def test_confusion_rows_window_and_sizes(dev, n):
    g = torch.Generator().manual_seed(n)
    K = 18
    x = ((torch.randn(n, K, generator=g) * 3).round() / 3).to(dev)
    t = torch.randint(0, K - 1, (n,), generator=g).to(dev)
    _check(x, t)
    _check(x, t, window=(1, K - 1), ignore=0, Kc=K - 1)                       # the lidar-seg update
    _check(x, t.to(torch.uint8), window=(1, K - 1), ignore=0, Kc=K - 1)
    _check(x.to(torch.bfloat16), t, window=(2, 9), Kc=10)


@gpu
def test_confusion_other_layouts_and_integer_predictions(dev):
    g = torch.Generator().manual_seed(4)
    K = 6
    x = _occ_view(2, K, dev, g=g, shape=(5, 7, 3))                 # planes, S % 4 != 0: one element per lane
    t = torch.randint(0, K, (2, 5, 7, 3), generator=g).to(dev)
    _check(x, t, (torch.rand(2, 5, 7, 3, generator=g) < 0.5).to(dev))
    _check(x[:, ::2], t[:, ::2])                                   # neither layout: copied
    xt = torch.randn(K, 300, generator=g).to(dev).t()              # [N, K] view of a [K, N] tensor
    _check(xt, torch.randint(0, K, (300,), generator=g).to(dev))
    p = torch.randint(-1, K + 1, (1000,), generator=g)             # integer predictions, some out of range
    tg = torch.randint(0, K, (1000,), generator=g)
    _check(p.to(dev), tg.to(dev), Kc=K)
    _check(p.to(dev).int(), tg.to(dev), Kc=K)


@gpu
def test_confusion_skewed_accumulating_and_invalid(dev):
    g = torch.Generator().manual_seed(5)
    K = 18
    vol = torch.randn(1, K, 200, 200, 16, generator=g)
    free = torch.rand(1, 200, 200, 16, generator=g) < 0.99
    vol[:, K - 1][free] = 100.0                                     # 99 % "free" predicted "free"
    t = torch.randint(0, K, (1, 200, 200, 16), generator=g)
    t[free] = K - 1
    x = vol.to(dev).permute(0, 2, 3, 4, 1)
    rcm = _check(x, t.to(dev))
    assert int(rcm[K - 1, K - 1]) > 0.98 * t.numel()
    # two updates accumulate
    state = _run(x, t.to(dev), Kc=K)
    _run(x, t.to(dev), Kc=K, state=state)
    assert torch.equal(state[0].cpu(), 2 * rcm) and int(state[1]) == 0
    # targets out of range land in `invalid`, not in the matrix
    tb = t.clone()
    tb[0, :3, 0, 0] = torch.tensor([-1, K, 255])
    cm, inv = _run(x, tb.to(dev), Kc=K)
    rcm2, rinv2 = ref_confmat(x, tb, None, None, K, None)
    assert int(inv) == 3 == rinv2 and torch.equal(cm.cpu(), rcm2)


@gpu
@pytest.mark.parametrize("P,R", [(3000, 3500), (2000, 600), (0, 40), (50, 1)])
def test_lidarseg_predict_bit_exact(dev, P, R):
    g = torch.Generator().manual_seed(P + R)
    K = 18
    logits = torch.randn(P, K, generator=g) * 10
    idx = torch.randint(0, R, (P,), generator=g)
    if P:
        idx[: P // 3] = idx[P // 3: 2 * (P // 3)].flip(0)           # repeats, out of point order
    labels, inv = ops.lidarseg_predict(logits.to(dev), idx.to(dev), R, (1, K - 1))
    assert labels.shape == (R,) and labels.dtype == torch.int64 and int(inv) == 0
    assert torch.equal(labels.cpu(), ref_lidarseg_labels(logits, idx, R, 1, K - 1))
    if P == 0:
        assert bool((labels == 1).all())                          # unmapped: zero logits -> lo
    # indices out of range are counted and not summed
    if P >= 10:
        bad = idx.clone()
        bad[:3] = torch.tensor([-1, R, R + 100])
        labels, inv = ops.lidarseg_predict(logits.to(dev), bad.to(dev), R, (1, K - 1))
        keep = (bad >= 0) & (bad < R)
        assert int(inv) == 3
        assert torch.equal(labels.cpu(), ref_lidarseg_labels(logits[keep], bad[keep], R, 1, K - 1))


def _val_outputs(cfg, batch, dev, g):
    pts = [torch.randn(len(p), cfg.num_classes, generator=g).to(dev) for p in batch[6]]
    occ = _occ_view(batch[11].shape[0], cfg.num_classes, dev, g=g)
    return pts, occ, None


@gpu
def test_update_val_never_synchronises_and_graph_replay(dev):
    cfg = dataclasses.replace(CFG_TINY, num_classes=18)
    batch = M.synthetic_val_batch(cfg, 2, seed=7, device=dev, num_points=500)
    outputs = _val_outputs(cfg, batch, dev, torch.Generator().manual_seed(7))
    ev = metrics.SegEvaluator(device=dev)
    ev.update_val(outputs, batch)                                   # warm-up: workspaces allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.update_val(outputs, batch)
        with pytest.raises(RuntimeError):                           # the reference's boolean index syncs
            outputs[1][batch[14]]
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert int(ev.occ_val_iou.confmat.sum()) == 2 * int(batch[14].sum())

    # one update captured in a graph, replayed three times
    j = metrics.JaccardIndex(18, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        j.update(outputs[1], batch[11], batch[14])
    torch.cuda.current_stream().wait_stream(s)
    once = j.confmat.clone()
    j.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        j.update(outputs[1], batch[11], batch[14])
    assert int(j.confmat.sum()) == 0
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(j.confmat, 3 * once) and int(once.sum()) == int(batch[14].sum())


@gpu
def test_evaluator_end_to_end_matches_reference(dev):
    """A small VAMPIRE2 on the GPU, two validation batches: SegEvaluator against the restated reference
    (base_exp.py:634-663 and :880-910; the index_add_ on the CPU as in :836), then the same for the training
    update (:370-382) on the 12 outputs of the training forward."""
    K = 6
    cfg = dataclasses.replace(CFG_TINY, density_mode="sdf", final_dim=(192, 224), num_classes=K)
    torch.manual_seed(0)
    bb, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(cfg.sdf_bias)
    names = ["other", "a", "b", "c", "d", "free"]
    ev = metrics.SegEvaluator(K, class_names=names, device=dev)
    rcm = torch.zeros(K - 1, K - 1, dtype=torch.int64)
    rocc = torch.zeros(K, K, dtype=torch.int64)
    for seed in (11, 12):
        batch = M.synthetic_val_batch(cfg, 2, seed=seed, device=dev, num_points=300)
        model.eval()
        with torch.no_grad():
            pts_logits, occ_logits, _ = model(batch[0], batch[1], inrange_pts=batch[6], lidar_seg=True)
        ev.update_val((pts_logits, occ_logits, None), batch)
        for logits, idx, lab in zip(pts_logits, batch[9], batch[8]):
            seg = ref_lidarseg_labels(logits, idx, len(lab), 1, K - 1)
            rcm += ref_confmat(seg, lab, Kc=K - 1, ignore_index=0)[0]
        rocc += ref_confmat(occ_logits, batch[11], batch[14], Kc=K)[0]
    assert torch.equal(ev.val_iou.confmat.cpu(), rcm) and int(ev.val_iou.invalid) == 0
    assert torch.equal(ev.occ_val_iou.confmat.cpu(), rocc)
    assert int(rcm.sum()) > 0 and int(rocc.sum()) > 0
    out = ev.epoch_end("val")
    assert out["val/mIoU"] == float(np.nanmean(ref_iou(rcm)[1:].numpy()))
    assert out["val/occ_mIoU"] == float(np.nanmean(ref_iou(rocc)[:-1].numpy()))

    # the training update on multitask_step's forward outputs
    batch = M.synthetic_batch(cfg, 2, seed=13, device=dev, num_points=300, num_boxes=6)
    model.train()
    with torch.no_grad():
        out12 = model(batch[0], batch[1], inrange_pts=batch[11], lidar_seg=False)
    assert len(out12) == 12
    ev.update_train(out12, batch)
    rcm = sum(ref_confmat(lg, lab, window=(1, K - 1), Kc=K - 1, ignore_index=0)[0]
              for lg, lab in zip(out12[8], batch[12]))
    rocc = ref_confmat(out12[10], batch[16], batch[19], Kc=K)[0]
    assert torch.equal(ev.train_iou.confmat.cpu(), rcm) and torch.equal(ev.occ_train_iou.confmat.cpu(), rocc)
    tr = ev.epoch_end("train")
    assert tr["train/mIoU"] == float(np.nanmean(ref_iou(rcm)[1:].numpy()))
    assert tr["train/occ_mIoU"] == float(np.nanmean(ref_iou(rocc)[:-1].numpy()))
