"""Detection scoring on the device (vampire_amd.metrics.DetEvaluator over the HIP matching kernel of
vampire_amd/csrc/det_eval.hip) against a float64 numpy restatement of the definition in DESIGN 8.19 (the published
nuScenes detection protocol `detection_cvpr_2019`; parity with the devkit is unpinned: it is not installed here).

The oracle below is written for this file and shares no code with the package: it matches class by class over the
whole epoch, as the protocol is usually written down, where the kernel works per (sample, class).  Inputs are built so
that its decisions are exact: centres, sizes and velocities are multiples of 1/64, scores multiples of 1/256 (equal
in fp32, bf16 and fp16), yaws arbitrary fp32; every squared distance is then exact in float64, ties are real ties and
a distance equal to a threshold or a class range is a real equality.

Tolerances.  AP, mAP and everything derived from counts: 1e-12 (integer counts combined in float64; only the order
of a few hundred additions can differ).  True-positive metrics and NDS: 16 * 2^-24 * max(1, |v|) (the records are
the same fp32 values on both sides; the margin covers float64 summation order and a contracted multiply-add ahead of
the fp32 rounding).  Record fields are compared exactly."""
import ctypes as C
import dataclasses
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi, _header, metrics              # noqa: E402
from vampire_amd import evaluation as E                      # noqa: E402
from vampire_amd import multitask as M                       # noqa: E402
from vampire_amd.build import build_library                  # noqa: E402
from vampire_amd.config import CFG_TINY                      # noqa: E402

NAMES = list(M.CLASSES)
CAR, BARRIER, PED, CONE = NAMES.index("car"), NAMES.index("barrier"), NAMES.index("pedestrian"), NAMES.index("traffic_cone")
BUS, BICYCLE = NAMES.index("bus"), NAMES.index("bicycle")
GT_CAP = 256
PREFIX = "pts_bbox_NuScenes"

# ----------------------------------------------------------------------------- the definition, restated in float64
RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40,
         "motorcycle": 40, "bicycle": 40, "traffic_cone": 30, "barrier": 30}
THS = (0.5, 1.0, 2.0, 4.0)
TH_TP = 2.0
ATTRS = ["cycle.with_rider", "cycle.without_rider", "pedestrian.moving", "pedestrian.standing",
         "pedestrian.sitting_lying_down", "vehicle.moving", "vehicle.parked", "vehicle.stopped"]
ERRS = ["trans_err", "scale_err", "orient_err", "vel_err", "attr_err"]
ERR_MEAN = {"trans_err": "mATE", "scale_err": "mASE", "orient_err": "mAOE", "vel_err": "mAVE", "attr_err": "mAAE"}


def o_pred_attr(name, vx, vy):
    """The speed rule of the reference's det_evaluators.py:254-274."""
    default = {"car": "vehicle.parked", "pedestrian": "pedestrian.moving", "trailer": "vehicle.parked",
               "truck": "vehicle.parked", "bus": "vehicle.moving", "motorcycle": "cycle.without_rider",
               "construction_vehicle": "vehicle.parked", "bicycle": "cycle.without_rider", "barrier": "",
               "traffic_cone": ""}
    if math.sqrt(vx * vx + vy * vy) > 0.2:
        if name in ("car", "construction_vehicle", "bus", "truck", "trailer"):
            return "vehicle.moving"
        if name in ("bicycle", "motorcycle"):
            return "cycle.with_rider"
        return default[name]
    if name == "pedestrian":
        return "pedestrian.standing"
    if name == "bus":
        return "vehicle.stopped"
    return default[name]


def o_errors(name, pb, gb, gattr):
    """The five errors of a match in float64 (pb, gb: rows of Python floats)."""
    nan = float("nan")
    out = dict.fromkeys(ERRS, nan)
    out["trans_err"] = math.sqrt((gb[0] - pb[0]) ** 2 + (gb[1] - pb[1]) ** 2)
    inter = min(gb[3], pb[3]) * min(gb[4], pb[4]) * min(gb[5], pb[5])
    vg, vp = gb[3] * gb[4] * gb[5], pb[3] * pb[4] * pb[5]
    out["scale_err"] = 1.0 - inter / (vg + vp - inter)
    if name != "traffic_cone":
        per = math.pi if name == "barrier" else 2 * math.pi
        d = (gb[6] - pb[6] + per / 2) % per - per / 2
        if d > math.pi:
            d -= 2 * math.pi
        out["orient_err"] = abs(d)
    if name not in ("traffic_cone", "barrier"):
        pv, gv = (pb[7:9], gb[7:9]) if len(pb) == 9 else ((0.0, 0.0), (0.0, 0.0))
        out["vel_err"] = math.sqrt((gv[0] - pv[0]) ** 2 + (gv[1] - pv[1]) ** 2)
        if gattr is not None and gattr >= 0:
            out["attr_err"] = 1.0 - float(ATTRS[gattr] == o_pred_attr(name, pv[0], pv[1]))
    return out


def o_match(samples, names=NAMES):
    """Filtering and matching over a list of samples (dicts of numpy arrays: boxes, scores, labels, gt_boxes, gt_labels,
    gt_attrs | None).  Returns per class {npos, preds: [(score, sample, row, tp bits, errors | None)] in match order}."""
    out = []
    for c, name in enumerate(names):
        preds, gts = [], {}
        for s, smp in enumerate(samples):
            gts[s] = []
            for g in range(len(smp["gt_labels"])):
                gb = [float(v) for v in smp["gt_boxes"][g]]
                if int(smp["gt_labels"][g]) == c and math.sqrt(gb[0] * gb[0] + gb[1] * gb[1]) < RANGE[name]:
                    gts[s].append((g, gb))
            for r in range(len(smp["labels"])):
                pb = [float(v) for v in smp["boxes"][r]]
                if int(smp["labels"][r]) == c and math.sqrt(pb[0] * pb[0] + pb[1] * pb[1]) < RANGE[name]:
                    preds.append((float(smp["scores"][r]), s, r, pb))
        # a NaN of either sign orders above every number and NaNs are equal among themselves (-0.0 == 0.0 as floats)
        order = [t[-1] for t in sorted((math.isnan(p[0]), 0.0 if math.isnan(p[0]) else p[0], i)
                                       for i, p in enumerate(preds))][::-1]
        bits = {i: 0 for i in order}
        errs = {i: None for i in order}
        for h, th in enumerate(THS):
            taken = set()
            for i in order:
                _, s, r, pb = preds[i]
                best, best_d2 = None, float("inf")
                for g, gb in gts[s]:
                    if (s, g) in taken:
                        continue
                    d2 = (gb[0] - pb[0]) ** 2 + (gb[1] - pb[1]) ** 2
                    if d2 < best_d2:
                        best, best_d2 = (g, gb), d2
                if best is not None and best_d2 < th * th:
                    taken.add((s, best[0]))
                    bits[i] |= 1 << h
                    if th == TH_TP:
                        ga = samples[s].get("gt_attrs")
                        errs[i] = o_errors(name, pb, best[1], None if ga is None else int(ga[best[0]]))
        out.append(dict(npos=sum(len(v) for v in gts.values()),
                        preds=[(preds[i][0], preds[i][1], preds[i][2], bits[i], errs[i]) for i in order]))
    return out


def o_cummean(x):
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).all():
        return np.ones(len(x))
    sums, counts = np.nancumsum(x), np.cumsum(~np.isnan(x))
    return np.divide(sums, counts, out=np.zeros_like(sums), where=counts != 0)


def o_scores(matched, names=NAMES, prefix=PREFIX):
    """Curves and scores from o_match's result; the recorded errors are rounded to fp32 first (part of the definition)."""
    out, aps, tp_by_err = {}, [], {e: [] for e in ERRS}
    for name, m in zip(names, matched):
        class_ap = []
        for h, th in enumerate(THS):
            tp = np.array([(p[3] >> h) & 1 for p in m["preds"]], dtype=bool)
            conf = np.array([p[0] for p in m["preds"]], dtype=np.float64)
            if m["npos"] == 0 or tp.sum() == 0:
                prec, cf, curves = np.zeros(101), np.zeros(101), {e: np.ones(101) for e in ERRS}
            else:
                tpc, fpc = np.cumsum(tp).astype(float), np.cumsum(~tp).astype(float)
                prec, rec = tpc / (fpc + tpc), tpc / float(m["npos"])
                grid = np.linspace(0, 1, 101)
                prec = np.interp(grid, rec, prec, right=0)
                cf = np.interp(grid, rec, conf, right=0)
                curves = {}
                if th == TH_TP:
                    mconf = conf[tp]
                    for e in ERRS:
                        vals = [float(np.float32(p[4][e])) for p in m["preds"] if p[4] is not None]
                        curves[e] = np.interp(cf[::-1], mconf[::-1], o_cummean(vals)[::-1])[::-1]
            ap = float(np.mean(np.maximum(prec[11:] - 0.1, 0))) / 0.9
            class_ap.append(ap)
            out[f"{prefix}/{name}_AP_dist_{th}"] = ap
            if th == TH_TP:
                nz = np.nonzero(cf)[0]
                last = nz[-1] if len(nz) else 0
                for e in ERRS:
                    if (name == "traffic_cone" and e in ("attr_err", "vel_err", "orient_err")) or \
                            (name == "barrier" and e in ("attr_err", "vel_err")):
                        v = float("nan")
                    elif last < 11:
                        v = 1.0
                    else:
                        v = float(np.mean(curves[e][11:last + 1]))
                    out[f"{prefix}/{name}_{e}"] = v
                    tp_by_err[e].append(v)
        aps.append(np.mean(class_ap))
    mean_ap = float(np.mean(aps))
    total = 5.0 * mean_ap
    for e in ERRS:
        v = float(np.nanmean(tp_by_err[e]))
        out[f"{prefix}/{ERR_MEAN[e]}"] = v
        total += max(1.0 - v, 0.0)
    out[f"{prefix}/NDS"] = total / 10.0
    out[f"{prefix}/mAP"] = mean_ap
    return out


# ----------------------------------------------------------------------------- exact inputs
def q64(rng, lo, hi, shape):
    """Multiples of 1/64 in [lo, hi]."""
    return (rng.integers(int(lo * 64), int(hi * 64) + 1, shape) / 64.0).astype(np.float32)


def sample(boxes, scores, labels, gt_boxes, gt_labels, gt_attrs=None, cols=9):
    f = lambda a, w: np.asarray(a, dtype=np.float32).reshape(-1, w)
    return dict(boxes=f(boxes, cols), scores=np.asarray(scores, dtype=np.float32), labels=np.asarray(labels, dtype=np.int64),
                gt_boxes=f(gt_boxes, cols), gt_labels=np.asarray(gt_labels, dtype=np.int64),
                gt_attrs=None if gt_attrs is None else np.asarray(gt_attrs, dtype=np.int8))


def box(x, y, yaw=0.0, dims=(2.0, 4.0, 1.5), vel=(0.0, 0.0), z=0.0, cols=9):
    return [x, y, z, *dims, yaw, *vel][:cols]


def random_scene(rng, n_gt, n_pred, classes, cols=9, attrs=True, spread=56.0, score_levels=24, on_ranges=True):
    """Ground truth scattered over +-spread m (some beyond the class ranges, some exactly on them), predictions at a
    ground-truth centre plus an offset that is often exactly a threshold; few score levels (ties); arbitrary yaws."""
    gtb = np.zeros((n_gt, cols), np.float32)
    gtb[:, :2] = q64(rng, -spread, spread, (n_gt, 2))
    on_range = [(50, 0), (0, -50), (30, 40), (-30, 0), (0, 30), (40, 0), (-24, -32), (18, 24)]
    for g in range(0, n_gt if on_ranges else 0, 5):
        gtb[g, :2] = on_range[rng.integers(len(on_range))]
    gtb[:, 2] = q64(rng, -2, 2, n_gt)
    gtb[:, 3:6] = q64(rng, 0.25, 8, (n_gt, 3))
    gtb[:, 6] = rng.uniform(-7, 7, n_gt).astype(np.float32)
    gtl = rng.choice(classes, n_gt)
    pb = np.zeros((n_pred, cols), np.float32)
    offs = np.array([(0, 0), (0.5, 0), (0, -0.5), (1, 0), (0, 1), (2, 0), (0, -2), (4, 0), (0, 4), (0.25, 0.25),
                     (1.5, 0.5), (-3, 1), (0.75, 0), (6, 6)], np.float32)
    src = rng.integers(0, max(n_gt, 1), n_pred)
    for r in range(n_pred):
        o = offs[rng.integers(len(offs))] if rng.random() < 0.6 else q64(rng, -3, 3, 2)
        pb[r, :2] = (gtb[src[r], :2] if n_gt else 0) + o
    pb[:, 2] = q64(rng, -2, 2, n_pred)
    pb[:, 3:6] = q64(rng, 0.25, 8, (n_pred, 3))
    pb[:, 6] = rng.uniform(-7, 7, n_pred).astype(np.float32)
    pl = np.where(rng.random(n_pred) < 0.8, gtl[src] if n_gt else rng.choice(classes, n_pred), rng.choice(classes, n_pred))
    if cols == 9:
        gtb[:, 7:9] = q64(rng, -2, 2, (n_gt, 2))
        pb[:, 7:9] = np.where(rng.random((n_pred, 1)) < 0.5, q64(rng, -2, 2, (n_pred, 2)), q64(rng, -0.125, 0.125, (n_pred, 2)))
    scores = (rng.integers(1, score_levels + 1, n_pred) * (256 // score_levels) / 256.0).astype(np.float32)
    gta = rng.integers(-1, 8, n_gt).astype(np.int8) if attrs else None
    return sample(pb, scores, pl, gtb, gtl, gta, cols)


# ----------------------------------------------------------------------------- device side helpers
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def det_result(samples, width, dev, score_dtype=torch.float32, counts=None, raw_scores=None):
    """raw_scores: a [B, width] tensor of score_dtype to hand over as it is (bit patterns a conversion from the samples'
    fp32 scores would not keep, such as a NaN's sign in bf16); the samples' scores are then its values in fp32."""
    B, cols = len(samples), samples[0]["boxes"].shape[1]
    boxes, scores = torch.zeros(B, width, cols), torch.zeros(B, width)
    labels, cnt = torch.zeros(B, width, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b, s in enumerate(samples):
        n = len(s["labels"])
        boxes[b, :n], scores[b, :n] = torch.from_numpy(s["boxes"]), torch.from_numpy(s["scores"])
        labels[b, :n], cnt[b] = torch.from_numpy(s["labels"]).int(), n
    if counts is not None:
        cnt = torch.tensor(counts, dtype=torch.int32)
    if raw_scores is not None:
        assert raw_scores.dtype == score_dtype and tuple(raw_scores.shape) == (B, width)
        assert torch.equal(raw_scores.float().isnan(), scores.isnan())       # (the samples' fp32 scores are its values;
        assert torch.equal(raw_scores.float().nan_to_num(7.0), scores.nan_to_num(7.0))     # a NaN's bits are the caller's)
    scores = scores.to(score_dtype) if raw_scores is None else raw_scores
    return E.DetResult(boxes.to(dev), scores.to(dev), labels.to(dev), cnt.to(dev))


def gt_lists(samples, dev, label_dtype=torch.int64):
    gb = [torch.from_numpy(s["gt_boxes"]).to(dev) for s in samples]
    gl = [torch.from_numpy(s["gt_labels"]).to(label_dtype).to(dev) for s in samples]
    ga = None if samples[0]["gt_attrs"] is None else [torch.from_numpy(s["gt_attrs"]).to(dev) for s in samples]
    return gb, gl, ga


def update(ev, samples, dev, width, **kw):
    gb, gl, ga = gt_lists(samples, dev, kw.pop("label_dtype", torch.int64))
    ev.update(det_result(samples, width, dev, **kw), gb, gl, ga)


def record_rows(ev, n_samples):
    return ev.state.records[:n_samples * ev.state.max_dets].cpu().numpy()


def on_f32_boundary(v):
    """True when the float64 value lies within one float64 ulp of the midpoint of two neighbouring fp32 values."""
    f = np.float32(v)
    for other in (np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))):
        mid = (float(f) + float(other)) / 2
        if abs(v - mid) <= np.spacing(mid):
            return True
    return False


def check_records(rows, samples, width, names=NAMES):
    """Every record field against the oracle; returns the oracle's match result.  The fp32 errors must be bit-equal;
    a difference is tolerated (and counted) only on an fp32 rounding boundary, and none is expected on these inputs."""
    matched = o_match(samples, names)
    want = {}
    for c, m in enumerate(matched):
        for score, s, r, bits, errs in m["preds"]:
            want[(s, r)] = (c, score, bits, errs)
    boundary = 0
    for s in range(len(samples)):
        for r in range(width):
            row = rows[s * width + r]
            if (s, r) not in want:
                assert not row.any(), f"sample {s} row {r}: expected an invalid (all-zero) record, got {row}"
                continue
            c, score, bits, errs = want[(s, r)]
            assert row[0] == samples[s]["scores"][r:r + 1].view(np.int32)[0], (s, r, "score")       # (a NaN's bits too)
            assert math.isnan(score) or np.float32(score) == samples[s]["scores"][r]
            assert row[1] == (c | 1 << 8 | bits << 16), (s, r, f"class/valid/tp word {row[1]:#x}, oracle class {c} bits {bits:#x}")
            assert row[7] == 0
            for k, e in enumerate(ERRS):
                v = float("nan") if errs is None else errs[e]
                got = row[2 + k:3 + k].view(np.float32)[0]
                if math.isnan(v):
                    assert math.isnan(got), (s, r, e, got)
                elif np.float32(v).view(np.int32) != row[2 + k]:
                    assert on_f32_boundary(v) and abs(float(got) - v) <= np.spacing(np.float32(v)), (s, r, e, got, v)
                    boundary += 1
    assert boundary == 0, f"{boundary} errors differ on an fp32 rounding boundary"
    return matched


def check_scores(got, want):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if math.isnan(w):
            assert math.isnan(g), k
        elif "_AP_dist_" in k or k.endswith("/mAP"):
            assert abs(g - w) <= 1e-12, (k, g, w)
        else:
            assert abs(g - w) <= 16 * 2.0 ** -24 * max(1.0, abs(w)), (k, g, w)


def run_case(samples, dev, width, max_samples=None, batches=None, names=NAMES, protocol=None, **kw):
    """Feed `samples` (in `batches` of the given sizes, default one) and hold records, npos and scores to the oracle.
    names: the evaluator's class list; protocol: DetEvaluator's keyword arguments (max_boxes_per_sample)."""
    ev = metrics.DetEvaluator(names, max_samples or len(samples), width, dev, **(protocol or {}))
    at = 0
    for n in batches or [len(samples)]:
        update(ev, samples[at:at + n], dev, width, **kw)
        at += n
    matched = check_records(record_rows(ev, len(samples)), samples, width, names)
    assert ev.state.state[8:8 + len(names)].tolist() == [m["npos"] for m in matched]
    check_scores(ev.compute(), o_scores(matched, names))
    return ev, matched


# ----------------------------------------------------------------------------- CPU: the oracle on hand-worked cases
def test_oracle_one_match_at_three_quarters_of_a_metre():
    s = sample([box(10.75, 5)], [0.5], [CAR], [box(10, 5)], [CAR])
    m = o_match([s])
    assert m[CAR]["npos"] == 1 and m[CAR]["preds"][0][3] == 0b1110
    assert m[CAR]["preds"][0][4]["trans_err"] == 0.75
    out = o_scores(m)
    assert out[f"{PREFIX}/car_AP_dist_0.5"] == 0.0
    for d in ("1.0", "2.0", "4.0"):
        assert abs(out[f"{PREFIX}/car_AP_dist_{d}"] - 1.0) <= 1e-12
    assert abs(out[f"{PREFIX}/car_trans_err"] - 0.75) <= 1e-12
    assert out[f"{PREFIX}/car_scale_err"] == 0.0 and out[f"{PREFIX}/car_orient_err"] == 0.0
    assert out[f"{PREFIX}/car_attr_err"] == 1.0               # no attribute on the ground truth: all NaN gives ones
    assert abs(out[f"{PREFIX}/mAP"] - 0.075) <= 1e-12          # one class of ten, three thresholds of four


def test_oracle_score_tie_goes_to_the_later_sample_then_the_higher_row():
    gt = ([box(0, 0)], [CAR])
    a = sample([box(0.25, 0), box(0.125, 0)], [0.5, 0.5], [CAR, CAR], *gt)
    m = o_match([a])[CAR]["preds"]
    assert [(p[2], p[3]) for p in m] == [(1, 0b1111), (0, 0)]            # row 1 first: it takes the box, row 0 is an FP
    b = sample([box(0.25, 0)], [0.5], [CAR], *gt)
    m = o_match([b, a])[CAR]["preds"]
    assert [(p[1], p[2]) for p in m] == [(1, 1), (1, 0), (0, 0)]          # the later sample first


def test_oracle_no_fallback_to_a_farther_free_box():
    """The nearest box is taken by a better prediction; the next one lies inside the threshold and stays free."""
    s = sample([box(0, 0), box(0.25, 0)], [0.9, 0.8], [CAR, CAR], [box(0, 0), box(1.5, 0)], [CAR, CAR])
    m = o_match([s])[CAR]["preds"]
    assert m[0][3] == 0b1111
    assert m[1][3] == 0b1100          # at 0.5 and 1 m its nearest free box is 1.25 m away; at 2 and 4 m it matches it
    s = sample([box(0, 0), box(0.25, 0)], [0.9, 0.8], [CAR, CAR], [box(0, 0), box(-1.5, 0)], [CAR, CAR])
    m = o_match([s])[CAR]["preds"]
    assert m[1][4]["trans_err"] == 1.75
    # chosen first, tested afterwards: the nearest FREE box is the only candidate
    s = sample([box(0, 0), box(3, 0)], [0.9, 0.8], [CAR, CAR], [box(0, 0), box(3.75, 0), box(8, 0)], [CAR] * 3)
    assert [p[3] for p in o_match([s])[CAR]["preds"]] == [0b1111, 0b1110]


def test_oracle_no_predictions_curve_and_nan_running_means():
    gt_only = sample([], [], [], [box(1, 1)], [PED])
    out = o_scores(o_match([gt_only]))
    assert out[f"{PREFIX}/pedestrian_AP_dist_2.0"] == 0.0 and out[f"{PREFIX}/pedestrian_trans_err"] == 1.0
    assert out[f"{PREFIX}/mAP"] == 0.0 and out[f"{PREFIX}/mATE"] == 1.0 and out[f"{PREFIX}/NDS"] == 0.0
    assert math.isnan(out[f"{PREFIX}/traffic_cone_vel_err"]) and math.isnan(out[f"{PREFIX}/barrier_attr_err"])
    assert out[f"{PREFIX}/barrier_orient_err"] == 1.0
    pred_only = sample([box(1, 1)], [0.5], [PED], [], [])
    assert o_scores(o_match([pred_only]))[f"{PREFIX}/pedestrian_AP_dist_4.0"] == 0.0
    assert np.array_equal(o_cummean([np.nan, np.nan]), [1.0, 1.0])
    assert np.array_equal(o_cummean([np.nan, 1.0, np.nan, 0.0]), [0.0, 1.0, 1.0, 0.5])
    # attributes: the first match's ground truth has none (NaN), the second's disagrees with the prediction
    s = sample([box(0, 0, vel=(1, 0)), box(10, 0)], [0.9, 0.8], [CAR, CAR], [box(0, 0), box(10, 0)], [CAR, CAR], [-1, 5])
    m = o_match([s])
    assert math.isnan(m[CAR]["preds"][0][4]["attr_err"]) and m[CAR]["preds"][1][4]["attr_err"] == 1.0   # parked != moving
    assert 0.0 < o_scores(m)[f"{PREFIX}/car_attr_err"] < 1.0     # the running mean goes from 0 (no finite value yet) to 1


def test_oracle_orientation_periods():
    e = o_errors("barrier", box(0, 0, yaw=0.0), box(0, 0, yaw=math.pi - 0.01), None)
    assert abs(e["orient_err"] - 0.01) < 1e-12                       # period pi for barriers
    e = o_errors("car", box(0, 0, yaw=0.0), box(0, 0, yaw=math.pi - 0.01), None)
    assert abs(e["orient_err"] - (math.pi - 0.01)) < 1e-12
    e = o_errors("car", box(0, 0, yaw=-6.0), box(0, 0, yaw=6.5), None)
    assert abs(e["orient_err"] - abs(12.5 - 4 * math.pi)) < 1e-12    # yaws outside (-pi, pi]
    assert math.isnan(o_errors("traffic_cone", box(0, 0), box(0, 0), 3)["orient_err"])


# ----------------------------------------------------------------------------- CPU: the C ABI
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _desc(**kw):
    st = E.DetEvalState(None, None, tuple(NAMES), 8, 12, tuple(float(RANGE[n]) for n in NAMES))
    d = st.desc(2, 5, 9, torch.float32, torch.int64, True)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(d, k)[v[0]] = v[1]
        else:
            setattr(d, k, v)
    return d


def test_descriptor_layout_matches_the_header(lib):
    assert C.sizeof(_capi.VampDetEvalDesc) == 408
    header = _header.read()
    fields = [(ctype, name) for name, ctype, _ in header.structs["VampDetEvalDesc"]]
    ctypes_of = {"double": C.c_double, "int32_t": C.c_int32}
    got = [(n, t._type_ if issubclass(t, C.Array) else t) for n, t in _capi.VampDetEvalDesc._fields_]
    assert got == [(n, ctypes_of[t]) for t, n in fields]
    for macro, pinned in (("MAX_CLASSES", 16), ("GT_CAP", 256), ("MAX_WIDTH", 2048), ("RECORD_BYTES", 32),
                          ("STATE_WORDS", 24)):
        value = header.constants[f"VAMP_DET_EVAL_{macro}"]
        assert getattr(_capi, f"VAMP_DET_EVAL_{macro}") == value == pinned
    assert _capi.VAMP_DET_EVAL_GT_CAP == GT_CAP >= 256


def test_descriptor_defaults(lib):
    d = _desc()
    assert lib.vamp_det_eval_supported(C.byref(d)) == 1
    assert lib.vamp_det_eval_record_bytes(C.byref(d)) == 8 * 12 * 32
    assert list(d.dist_ths) == list(THS) and d.dist_th_tp == TH_TP and d.max_boxes_per_sample == 500
    assert [d.class_range[c] for c in range(10)] == [float(RANGE[n]) for n in NAMES]
    flags = {n: d.class_flags[c] for c, n in enumerate(NAMES)}
    assert flags["traffic_cone"] == 0 and flags["barrier"] == 3 and flags["car"] == 14
    for c, n in enumerate(NAMES):
        mv, st = o_pred_attr(n, 1.0, 0.0), o_pred_attr(n, 0.0, 0.0)
        assert d.attr_moving[c] == (ATTRS.index(mv) if mv else -1) and d.attr_still[c] == (ATTRS.index(st) if st else -1)


@pytest.mark.parametrize("change,message", [
    (dict(B=0), b"B must be"), (dict(M=0), b"M must be"), (dict(M=2049), b"M must be"), (dict(G=-1), b"G must be"),
    (dict(box_cols=8), b"box_cols"), (dict(score_dtype=_capi.VAMP_I64), b"score_dtype"),
    (dict(gt_label_dtype=_capi.VAMP_F32), b"gt_label_dtype"), (dict(has_attrs=2), b"has_attrs"),
    (dict(num_classes=0), b"num_classes"), (dict(num_classes=17), b"num_classes"),
    (dict(max_boxes_per_sample=0), b"max_boxes_per_sample"), (dict(max_samples=0), b"max_samples"),
    (dict(max_samples=1 << 30), b"max_samples"), (dict(class_range=(3, 0.0)), b"class_range"),
    (dict(class_range=(0, float("nan"))), b"class_range"), (dict(class_flags=(2, 16)), b"class_flags"),
    (dict(attr_moving=(1, 128)), b"attr_moving"), (dict(dist_ths=(1, 0.25)), b"ascend"),
    (dict(dist_ths=(0, 0.0)), b"dist_ths"), (dict(dist_th_tp=3.0), b"dist_th_tp"), (dict(reserved=(1, 7)), b"reserved")])
def test_bad_descriptors_are_rejected_without_gpu(lib, change, message):
    d = _desc(**change)
    assert lib.vamp_det_eval_supported(C.byref(d)) == 0
    assert lib.vamp_det_eval_record_bytes(C.byref(d)) == 0
    assert lib.vamp_det_eval_update(C.byref(d), *[None] * 10) == -1
    assert message in lib.vamp_last_error(), lib.vamp_last_error()


def test_null_pointers_and_cpu_tensors_are_refused(lib):
    d = _desc()
    assert lib.vamp_det_eval_update(C.byref(d), *[None] * 10) == -1
    assert b"pointer is NULL" in lib.vamp_last_error()
    assert lib.vamp_det_eval_supported(None) == 0 and lib.vamp_det_eval_record_bytes(None) == 0
    st = E.DetEvalState(None, None, tuple(NAMES), 8, 12, tuple(float(RANGE[n]) for n in NAMES))
    det = E.DetResult(torch.zeros(1, 12, 9), torch.zeros(1, 12), torch.zeros(1, 12, dtype=torch.int32),
                      torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_capi.VampireHipError):
        E.det_eval_update(st, det, [torch.zeros(0, 9)], [torch.zeros(0, dtype=torch.int64)])
    with pytest.raises(TypeError):
        E.det_eval_update(st, (det.boxes, det.scores), [], [])


def test_synthetic_val_batch_ground_truth_boxes():
    cfg = dataclasses.replace(CFG_TINY, num_classes=6)
    a = M.synthetic_val_batch(cfg, 2, seed=3, num_points=20)
    b = M.synthetic_val_batch(cfg, 2, seed=3, num_points=20, num_boxes=5)
    assert len(a) == len(b) == 15
    assert [tuple(x.shape) for x in a[4]] == [(12, 9)] * 2 and [tuple(x.shape) for x in b[4]] == [(5, 9)] * 2
    assert [tuple(x.shape) for x in b[5]] == [(5,)] * 2


# ----------------------------------------------------------------------------- GPU: records and scores against the oracle
@gpu
def test_record_bytes_mixed(dev):
    """B = 2, ten classes, M = 12: ties in score and distance, distances equal to thresholds and ranges, boxes beyond
    the ranges, attributes, arbitrary yaws -- every record field against the oracle."""
    rng = np.random.default_rng(1)
    for trial in range(6):
        samples = [random_scene(rng, 9, 12 - b, list(range(10)), score_levels=4) for b in range(2)]
        run_case(samples, dev, 12)
    samples = [random_scene(rng, 14, 12, [CAR, BARRIER, CONE], score_levels=2) for _ in range(2)]
    _, matched = run_case(samples, dev, 12)
    assert sum(p[3] != 0 for m in matched for p in m["preds"]) > 0


@gpu
def test_per_threshold_taken_sets(dev):
    """The first prediction takes box 0 at 2 m and 4 m only; the second then matches box 0 at 0.5 m and 1 m, nothing at
    2 m (box 0 is taken, box 1 is 2.75 m away) and box 1 at 4 m."""
    s = sample([box(1.5, 0), box(0.25, 0)], [0.875, 0.75], [CAR, CAR], [box(0, 0), box(3, 0)], [CAR, CAR])
    ev, matched = run_case([s], dev, 4)
    assert [p[3] for p in matched[CAR]["preds"]] == [0b1100, 0b1011]
    rows = record_rows(ev, 1)
    assert [int(rows[r, 1]) >> 16 for r in (0, 1)] == [0b1100, 0b1011]
    assert rows[0, 2:3].view(np.float32)[0] == 1.5 and math.isnan(rows[1, 2:3].view(np.float32)[0])


@gpu
def test_score_and_distance_ties(dev):
    """Equal scores: the later sample, then the higher row, goes first.  Equal distances: the lowest ground-truth row."""
    gt = ([box(0, 0), box(0.5, 0)], [CAR, CAR])
    a = sample([box(0.25, 0), box(0.25, 0), box(0.125, 0)], [0.5, 0.5, 0.5], [CAR] * 3, *gt)
    ev, matched = run_case([a, a], dev, 3)
    assert [(p[1], p[2]) for p in matched[CAR]["preds"]] == [(1, 2), (1, 1), (1, 0), (0, 2), (0, 1), (0, 0)]
    rows = record_rows(ev, 2)
    # row 2 takes box 0 (0.125 m); row 1, 0.25 m from both boxes, gets the lower free row: box 1; row 0 is left over
    assert [int(rows[r, 1]) >> 16 for r in range(3)] == [0, 0b1111, 0b1111]
    b = sample([box(0.25, 0)], [0.5], [CAR], [box(0, 0, dims=(1, 1, 1)), box(0.5, 0)], [CAR, CAR])
    ev, _ = run_case([b], dev, 3)
    assert record_rows(ev, 1)[0, 3:4].view(np.float32)[0] == np.float32(1 - 1 / 12)     # matched to box 0 (1 x 1 x 1)


@gpu
def test_empty_and_one_sided_classes(dev):
    rng = np.random.default_rng(2)
    full = random_scene(rng, 8, 10, [CAR, PED])
    no_dets = dict(full, boxes=full["boxes"][:0], scores=full["scores"][:0], labels=full["labels"][:0])
    no_gt = dict(full, gt_boxes=full["gt_boxes"][:0], gt_labels=full["gt_labels"][:0], gt_attrs=full["gt_attrs"][:0])
    gt_only = sample([], [], [], [box(1, 1), box(5, 5)], [BUS, BUS], [7, 7])          # a class with GT, no predictions
    pred_only = sample([box(1, 1), box(2, 2)], [0.5, 0.25], [BICYCLE] * 2, [], [], [])   # predictions, no GT anywhere
    ev, matched = run_case([full, no_dets, no_gt, gt_only, pred_only], dev, 10)
    assert matched[BUS]["npos"] == 2 and not matched[BUS]["preds"]
    assert matched[BICYCLE]["npos"] == 0 and len(matched[BICYCLE]["preds"]) == 2
    out = ev.compute()
    assert out[f"{PREFIX}/bus_AP_dist_4.0"] == 0.0 and out[f"{PREFIX}/bicycle_trans_err"] == 1.0
    run_case([no_gt, no_gt], dev, 10)                                                  # no ground truth at all: G = 0
    run_case([no_dets], dev, 10)


@gpu
@pytest.mark.parametrize("n_gt", [1, 63, 64, 65, GT_CAP])
def test_ground_truth_per_class_sizes(dev, n_gt):
    """Ground truth of one class in one sample: one lane, a full wave's first boxes, the LDS cap."""
    rng = np.random.default_rng(n_gt)
    s = random_scene(rng, n_gt, 40, [PED], spread=20.0, on_ranges=False)
    other = random_scene(rng, 3, 5, [PED, CAR], spread=20.0)
    _, matched = run_case([s, other], dev, 40)
    assert n_gt <= matched[PED]["npos"] <= n_gt + 3


@gpu
def test_ground_truth_over_the_cap_raises_at_compute(dev):
    rng = np.random.default_rng(5)
    s = random_scene(rng, GT_CAP + 1, 4, [PED], spread=20.0, on_ranges=False)
    ev = metrics.DetEvaluator(NAMES, 2, 4, dev)
    update(ev, [s], dev, 4)
    with pytest.raises(ValueError, match="ground-truth boxes"):
        ev.compute()


@gpu
@pytest.mark.parametrize("n_pred,width", [(1, 498), (64, 498), (65, 498), (498, 498)])
def test_predictions_per_class_sizes(dev, n_pred, width):
    """Predictions of one class: one, a wave, a wave and one, and the whole width (every trip of the rank pass)."""
    rng = np.random.default_rng(n_pred)
    s = random_scene(rng, 30, n_pred, [CAR], spread=30.0, score_levels=32)
    other = random_scene(rng, 10, 7, list(range(10)))
    _, matched = run_case([s, other], dev, width)
    assert len(matched[CAR]["preds"]) >= n_pred * 3 // 4


@gpu
def test_class_special_cases(dev):
    """Barrier yaw differences near pi / 2 and pi, yaws outside (-pi, pi], the NaN columns of traffic_cone and
    barrier, and ground-truth attributes given and omitted."""
    f = np.float32
    yaws = [(0.0, math.pi / 2), (0.0, math.pi / 2 + 1e-3), (0.0, math.pi / 2 - 1e-3), (0.0, math.pi), (0.0, math.pi - 1e-3),
            (3.0, -3.0), (-6.0, 6.5), (7.0, -7.0), (float(f(math.pi)), float(-f(math.pi))), (1e-3, -1e-3)]
    for cls, attr in ((BARRIER, 3), (CAR, 6), (CONE, -1), (PED, 3)):
        # five metres apart (more than the widest threshold), all ten inside the 30 m of barriers and cones
        pb = [box(5.0 * i - 22.25, 2.0, yaw=p, vel=(0.5 * (i % 2), 0.0)) for i, (p, g) in enumerate(yaws)]
        gb = [box(5.0 * i - 22.5, 2.0, yaw=g, vel=(0.25, 0.25)) for i, (p, g) in enumerate(yaws)]
        n = len(yaws)
        scores = [(200 - i) / 256 for i in range(n)]
        for attrs in ([attr] * n, None):
            s = sample(pb, scores, [cls] * n, gb, [cls] * n, attrs)
            ev, matched = run_case([s], dev, n)
            assert all(p[3] == 0b1111 for p in matched[cls]["preds"])
            rows = record_rows(ev, 1)
            errs = rows[:, 2:7].copy().view(np.float32)
            if cls == CONE:
                assert np.isnan(errs[:, 2:]).all() and not np.isnan(errs[:, :2]).any()
            elif cls == BARRIER:
                assert np.isnan(errs[:, 3:]).all() and not np.isnan(errs[:, :3]).any()
                assert (errs[:, 2] <= f(math.pi / 2) + 1e-6).all()
            else:
                assert not np.isnan(errs[:, :4]).any() and np.isnan(errs[:, 4]).all() == (attrs is None)


@gpu
@pytest.mark.parametrize("cols,score_dtype,label_dtype", [(7, torch.float32, torch.int64), (9, torch.bfloat16, torch.int32),
                                                          (9, torch.float16, torch.int64), (7, torch.bfloat16, torch.int32)])
def test_input_forms(dev, cols, score_dtype, label_dtype):
    rng = np.random.default_rng(cols)
    samples = [random_scene(rng, 12, 20, list(range(10)), cols=cols, score_levels=8) for _ in range(2)]
    ev, matched = run_case(samples, dev, 20, score_dtype=score_dtype, label_dtype=label_dtype)
    if cols == 7:
        vel = [p[4]["vel_err"] for c, m in enumerate(matched) if c not in (BARRIER, CONE) for p in m["preds"]
               if p[4] is not None]
        assert vel and all(v == 0.0 for v in vel)


@gpu
def test_batching_reset_and_errors(dev):
    rng = np.random.default_rng(9)
    samples = [random_scene(rng, 10, 16, list(range(10)), score_levels=6) for _ in range(4)]
    one, _ = run_case(samples, dev, 16)
    two, _ = run_case(samples, dev, 16, batches=[2, 2])
    want = record_rows(one, 4).copy()
    assert np.array_equal(record_rows(two, 4), want) and torch.equal(one.state.state, two.state.state)
    assert int(one.state.state[0]) == 4
    scores = one.compute()
    one.reset()
    assert int(one.state.state.abs().sum()) == 0
    update(one, samples, dev, 16)
    assert np.array_equal(record_rows(one, 4), want)
    check_scores(one.compute(), scores)

    def raises_at_compute(ev, pattern):
        torch.cuda.synchronize()                     # nothing raised so far: the update only counted
        with pytest.raises(ValueError, match=pattern):
            ev.compute()
        with pytest.raises(ValueError, match=pattern):
            ev.compute()                             # and it keeps raising until reset()
        ev.reset()
        update(ev, samples[:1], dev, ev.state.max_dets)
        ev.compute()

    # a detection label outside the class list, then a ground-truth label outside it
    ev = metrics.DetEvaluator(NAMES, 4, 16, dev)
    bad = dict(samples[0], labels=np.where(np.arange(16) == 3, 10, samples[0]["labels"]))
    update(ev, [samples[1], bad], dev, 16)
    assert ev.state.state[1:5].tolist() == [0, 0, 1, 0]
    raises_at_compute(ev, "outside the class list")
    bad = dict(samples[0], gt_labels=np.where(np.arange(10) == 2, 11, samples[0]["gt_labels"]))
    update(ev, [bad], dev, 16)
    raises_at_compute(ev, "1 labels outside the class list")
    # a full buffer: the third batch does not fit, its records are dropped
    ev = metrics.DetEvaluator(NAMES, 4, 16, dev)
    for _ in range(3):
        update(ev, samples[:2], dev, 16)
    assert ev.state.state[:5].tolist() == [6, 0, 0, 0, 1]
    assert np.array_equal(record_rows(ev, 2), want[:32])
    raises_at_compute(ev, "beyond max_samples")
    # counts[b] above max_boxes_per_sample
    ev = metrics.DetEvaluator(NAMES, 2, 502, dev)
    big = random_scene(rng, 10, 501, [CAR], spread=30.0)
    update(ev, [big], dev, 502)
    assert ev.state.state[1:5].tolist() == [1, 0, 0, 0]
    raises_at_compute(ev, "more than max_boxes_per_sample")
    update(ev, [dict(big, boxes=big["boxes"][:500], scores=big["scores"][:500], labels=big["labels"][:500])], dev, 502)
    ev.compute()                                     # 500 boxes are allowed


@gpu
def test_update_does_not_synchronise(dev):
    rng = np.random.default_rng(11)
    samples = [random_scene(rng, 10, 16, list(range(10))) for _ in range(2)]
    ev = metrics.DetEvaluator(NAMES, 4, 16, dev)
    det = det_result(samples, 16, dev)
    gb, gl, ga = gt_lists(samples, dev)
    ev.update(det, gb, gl, ga)                       # (first call: library load, allocator warm-up)
    ev.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.update(det, gb, gl, ga)
        ev.update(det, gb, gl, None)
        ev.reset()
        ev.update(det, gb, gl, ga)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    check_records(record_rows(ev, 2), samples, 16)


@gpu
def test_graph_replay_appends(dev):
    """One capture of update() on a single stream, replayed twice with changed contents: two batches appended, equal
    to the eager ones."""
    rng = np.random.default_rng(12)
    batches = [[random_scene(rng, 10, 16, list(range(10)), score_levels=5) for _ in range(2)] for _ in range(2)]
    pad = torch.nn.utils.rnn.pad_sequence

    def packed(samples):
        gb, gl, ga = gt_lists(samples, dev)
        out = [pad(gb, batch_first=True), pad(gl, batch_first=True, padding_value=-1), pad(ga, batch_first=True, padding_value=-1)]
        return det_result(samples, 16, dev), out

    eager = metrics.DetEvaluator(NAMES, 4, 16, dev)
    for samples in batches:
        det, gt = packed(samples)
        eager.update(det, *gt)
    ev = metrics.DetEvaluator(NAMES, 4, 16, dev)
    det, gt = packed(batches[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.update(det, *gt)
    torch.cuda.current_stream().wait_stream(s)
    ev.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ev.update(det, *gt)
    assert int(ev.state.state[0]) == 0               # capturing ran nothing
    for samples in batches:
        fresh_det, fresh_gt = packed(samples)
        fields = ("boxes", "scores", "labels", "counts")
        for dst, src in zip([getattr(det, f) for f in fields] + gt, [getattr(fresh_det, f) for f in fields] + fresh_gt):
            dst.copy_(src)
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ev.state.state, eager.state.state) and int(ev.state.state[0]) == 4
    assert torch.equal(ev.state.records, eager.state.records)
    check_records(record_rows(ev, 4), batches[0] + batches[1], 16)
    check_scores(ev.compute(), eager.compute())


@gpu
def test_end_to_end_test_step(dev):
    """synthetic_val_batch through DetEvaluator.test_step on the tiny configuration; the oracle is fed with
    DetResult.to_list()."""
    cfg = dataclasses.replace(CFG_TINY, density_mode="sdf", final_dim=(192, 224), num_classes=6)
    torch.manual_seed(0)
    bb, hd = M.reference_confs(cfg, output_channels=8, small_encoder=True)
    model = M.VAMPIRE2(bb, hd).to(dev)
    with torch.no_grad():
        model.backbone.density_conv.bias.fill_(cfg.sdf_bias)
    width = len(hd["tasks"]) * hd["test_cfg"]["post_max_size"]
    ev = metrics.DetEvaluator(NAMES, 2, width, dev)
    batch = M.synthetic_val_batch(cfg, 2, seed=21, device=dev, num_points=40, num_boxes=30)
    model.train()
    det = ev.test_step(model, batch)
    assert model.training                            # test_step puts the mode back
    samples = [sample(bx.cpu().numpy(), sc.float().cpu().numpy(), lb.cpu().numpy(), gb.cpu().numpy(), gl.cpu().numpy())
               for (bx, sc, lb), gb, gl in zip(det.to_list(), batch[4], batch[5])]
    assert sum(len(s["labels"]) for s in samples) > 0
    matched = check_records(record_rows(ev, 2), samples, width)
    print("end to end:", sum(len(s["labels"]) for s in samples), "detections,",
          sum(p[3] != 0 for m in matched for p in m["preds"]), "matched at some threshold")
    assert ev.state.state[8:18].tolist() == [m["npos"] for m in matched]
    check_scores(ev.compute(), o_scores(matched))
