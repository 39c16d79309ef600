"""Calls of DIFFERENT descriptors on one HotPath: a full batch, the partial last batch of an epoch, a full batch again.

The lift and render workspaces are kept per HotPath and grow only; the cell counters inside (`cnt`) lie behind regions
whose sizes follow B, N, C, fH and fW (lift_common.hpp: lift_workspace, render_common.hpp: cam_workspace).  "The
counters are zero" -- what VAMP_LIFTFWD_CELLS_CLEAN, VAMP_CAMPREP_COUNTERS_CLEAN and VAMP_RENDERFWD_COUNTERS_CLEAN
promise -- is therefore a fact about one layout of one buffer (ops.CounterState).  Every other sweep of the suite runs
its operator on a fresh HotPath or repeats one descriptor.

CPU part: a shadow model of a workspace buffer (which 256-byte blocks may be non-zero) is driven together with the
state object through a mirror of HotPath's bookkeeping (`Sim`); regions come from the library's own layout functions,
what each call writes from WRITES below.  The new state never promises over bytes the model has non-zero; the rule of
the commit before ("clean iff the key is not in the dirty set", ParentRule) does, on B = 2, 1, 2 and B = 4, 1, 4; and
each sequence's hazard is the overlap the layout functions give today.

GPU part (vamp_debug_checks(1) throughout: a wrong promise is refused, not relied on): the same sequences on one
HotPath, every step against the float64 oracle at the bar of its single-call sweep (tests/test_render_shape_sweep.py),
the recorded *_CLEAN flags equal to what `Sim` gives.  About 2 s on an MI355X, the oracles on the CPU included.

The cell-list lift backward writes no `gfeat_cl` (only the v1 splat does, lift.hip:1140-1157): of the overlaps in
HAZARDS, the one of B 2 -> 1 is harmless on the default path; the returns to the larger batch are not."""
import collections
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from oracle import aten_oracle as O
from vampire_amd import _capi, synthetic
from vampire_amd.config import CFG_TINY
from vampire_amd.geometry import PathGeometry, lift_matrices
from vampire_amd.ops import CounterState, lift_desc, render_desc
from test_hip_parity import NAMES, hot, _upstream
import test_render_shape_sweep as RS
from test_render_shape_sweep import (BETA_BAR, GRAD_BAR, LIFT_BAR, LIFT_GRAD_BAR, OUT_BAR, PATHS, VOLS, _Calls, library,
                                     oracle_render, rel_err, scene)

F64 = torch.float64
CFG = dataclasses.replace(CFG_TINY, density_mode="sdf")
NCAM = CFG.num_cams


# ---------------------------------------------------------------------------------------------------- layouts (CPU)
@functools.lru_cache(maxsize=None)
def lift_regions(B, C_=4):
    """({region: (offset, bytes)}, total bytes) of the lift workspace of CFG_TINY at B samples, C_ channels."""
    d, out = lift_desc(CFG, B, NCAM, C_, _capi.VAMP_F32), _capi.VampLiftWorkspaceLayout()
    assert library().vamp_lift_workspace_layout(C.byref(d), C.byref(out)) == 0
    return {r: (out.offset[i], out.bytes[i]) for i, r in enumerate(_capi.LIFTWS_REGIONS)}, out.total_bytes


@functools.lru_cache(maxsize=None)
def render_regions(B, bf16=False):
    """The same of the render workspace, the sample rows included (what a training call asks for)."""
    d = render_desc(CFG, B, NCAM, _capi.VAMP_BF16 if bf16 else _capi.VAMP_F32)
    out = _capi.VampRenderWorkspaceLayout()
    assert library().vamp_render_workspace_layout(C.byref(d), C.byref(out)) == 0
    return {r: (out.offset[i], out.bytes[i]) for i, r in enumerate(_capi.RENDERWS_REGIONS)}, out.bytes_with_rows


def under_cnt(new, old):
    """Regions of the layout `old` that the counters of the layout `new` lie over."""
    o, n = new["cnt"]
    return [r for r, (a, b) in old.items() if b and a < o + n and o < a + b]


# What a call leaves non-zero in the workspace, by region, and what it has zeroed when it ends: (writes, zeroes).
CELL_LISTS = _capi.RENDERWS_REGIONS[3:16]       # cnt .. records: "the 13 cell-list regions", render_common.hpp:291
WRITES = {
    # ---- lift (region comments: lift_common.hpp:126-134, 137-147)
    "lift-prologue": (("feat_cl", "cull"), ()),             # channel-FIRST features only: lift.hip:1086-1104 (w.feat_cl, w.cull);
                                                            # channel-last features: no first launch, lift.hip:1019-1035
    "lift-emit": (("cnt", "amask", "ptaps", "pcell"), ()),  # grad mode (EMIT_PAIRS): lift_common.hpp:229 (lift_emit_of), lift.hip:1064-1070
    "lift-scan": (("off", "bsum", "boff", "aux"), ("cnt",)),  # lift_bwd_cell.hip:697; "the scan zeroes what it has read", vampire_hip.h:119-122
    "lift-fill-gather": (("recs", "rowq"), ("cnt",)),       # lift_bwd_cell.hip:760 (fill: cnt as cursors), :783 (the gather re-zeroes them)
    "lift-splat": (("feat_cl", "gfeat_cl"), ()),            # the v1 backward, channel-first features: lift.hip:1140-1157
    # ---- render (render_common.hpp:288-294: "The forwards touch packed, term and rows (a forward that draws the
    # ranks: cnt, rank, tile_se too), the prepare pass the cell lists, the backward everything")
    "render-merged-train": (("term", "rows", "cnt", "rank", "tile_se"), ()),   # render_fwd_merged.hip:219-231, cam_rank_refs
    "render-direct-nograd": (("term",), ()),                # the one kernel makes no packed copy: ops.py ctx.packed
    "render-planned": (("packed", "term", "rows"), ()),     # copy + march: render_fwd.hip:602, 638
    "render-prepare": (CELL_LISTS, ("cnt",)),               # rank + scan, or the scan alone: render_bwd_cell.hip:388-407
    "render-backward": (("gcl",) + CELL_LISTS + ("beta_part",), ("cnt",)),      # render_bwd.hip:505; its own prepare: render_bwd_ray.hip:266-268
    "render-backward-v1": (("grad",), ()),                  # the splat's gradient copy over gcl .. beta_part: render_common.hpp:290
}


class Shadow:
    """One workspace buffer: which of its 256-byte blocks may be non-zero (every region is 256-byte aligned)."""

    def __init__(self, nbytes):
        self.nbytes, self.dirty = nbytes, np.zeros((nbytes + 255) // 256, dtype=bool)

    def _blocks(self, rng):
        assert rng[0] % 256 == 0 and rng[0] + rng[1] <= self.nbytes, (rng, self.nbytes)
        return slice(rng[0] // 256, (rng[0] + rng[1] + 255) // 256)

    def apply(self, regions, kind):
        writes, zeroes = WRITES[kind]
        for r in writes:
            self.dirty[self._blocks(regions[r])] = True
        for r in zeroes:
            self.dirty[self._blocks(regions[r])] = False

    def zero(self, rng):
        self.dirty[self._blocks(rng)] = False

    def is_zero(self, rng):
        return not self.dirty[self._blocks(rng)].any()


class ParentRule:
    """The rule of the commit before CounterState: clean iff the key is not in the dirty set."""

    def __init__(self):
        self.dirty = set()

    def fresh(self, key, addr):
        self.dirty.discard(key)

    def use(self, key, addr, rng):
        pass

    def begin(self, key, addr, rng):
        clean = key not in self.dirty
        self.dirty.add(key)
        return clean

    def done(self, key, addr, rng):
        self.dirty.discard(key)

    def spoil(self, key):
        self.dirty.add(key)


Promise = collections.namedtuple("Promise", "op desc promised zero")      # zero: the model has the counters zero


class Sim:
    """HotPath's bookkeeping around the counters (ops.py: _workspace, _finish_lift_scan, _LiftFn, _RenderFn) over
    shadow buffers: `rule` decides the promises, the shadows say whether they hold.  log: one Promise per counting pass."""

    def __init__(self, rule):
        self.rule, self.buf, self.log = rule, {}, []
        self.pending = None                         # a deferred lift scan: (addr, shadow, regions)
        self.lift_gen = self.pack_gen = self.allocs = 0

    def _ws(self, key, regions, total):
        b = self.buf.get(key)
        if b is None or b[1].nbytes < total:
            self.allocs += 1
            b = self.buf[key] = (4096 * self.allocs, Shadow(total))     # a new address
            self.rule.fresh(key, b[0])
        self.rule.use(key, b[0], regions["cnt"])
        return b

    def _count(self, op, desc, key, addr, sh, regions):
        promised = self.rule.begin(key, addr, regions["cnt"])
        self.log.append(Promise(op, desc, promised, sh.is_zero(regions["cnt"])))
        if not promised:
            sh.zero(regions["cnt"])                 # no promise: the library zero-fills

    # ---- lift
    def finish_lift_scan(self):
        p, self.pending = self.pending, None
        if p is not None:
            addr, sh, regions = p
            sh.apply(regions, "lift-scan")
            self.rule.done("lift", addr, regions["cnt"])

    def lift_forward(self, B, C_=4, grad=True, cl=False, defer=True, raises=False):
        regions, total = lift_regions(B, C_)
        addr, sh = self._ws("lift", regions, total)
        self.lift_gen += 1
        if grad:
            self.finish_lift_scan()
            self._count("lift", (B, C_), "lift", addr, sh, regions)
        if not cl:
            sh.apply(regions, "lift-prologue")
        if not grad:
            return None
        sh.apply(regions, "lift-emit")
        if raises:                                  # between the kernel and the scan
            return None
        if defer:
            self.pending = (addr, sh, regions)
        else:
            sh.apply(regions, "lift-scan")
            self.rule.done("lift", addr, regions["cnt"])
        return (self.lift_gen, addr)

    def lift_backward(self, B, C_, key, v1=False):
        regions, total = lift_regions(B, C_)
        addr, sh = self._ws("lift", regions, total)
        self.finish_lift_scan()
        fresh = key == (self.lift_gen, addr)
        self.lift_gen += 1
        self.rule.begin("lift", addr, regions["cnt"])
        if v1:
            sh.apply(regions, "lift-splat")
            return
        if not fresh:                               # the backward's own prepare pass: zero fill, count, scan
            sh.zero(regions["cnt"])
            sh.apply(regions, "lift-emit")
            sh.apply(regions, "lift-scan")
        sh.apply(regions, "lift-fill-gather")
        self.rule.done("lift", addr, regions["cnt"])

    # ---- render
    def render_forward(self, B, path="merged", grad=True, raises=False):
        """path: "merged" (ranks drawn by the launch, then the scan) | "planned" (copy + march, a full prepare pass) |
        "v1" (no prepare pass in the forward).  raises: at the prepare pass."""
        regions, total = render_regions(B)
        addr, sh = self._ws("render", regions, total)
        self.pack_gen += 1
        key = (self.pack_gen, addr)
        if not grad:
            sh.apply(regions, "render-planned" if path == "planned" else "render-direct-nograd")
            return None
        if path == "v1":
            sh.apply(regions, "render-direct-nograd")
            sh.apply(regions, "render-planned")     # (the rows; no packed copy in fact: a superset)
            return key + (False,)
        if path == "merged":
            self._count("render", B, "render", addr, sh, regions)
            sh.apply(regions, "render-merged-train")
        else:
            sh.apply(regions, "render-planned")
            self._count("render", B, "render", addr, sh, regions)      # (_cam_clean_flag is asked in front of the call)
        if raises:
            return None
        if self.pending is not None:                # vamp_render_camera_prepare_with_lift: both scans in one launch
            self.finish_lift_scan()
        if path != "merged":
            sh.dirty[sh._blocks(regions["cnt"])] = True                 # the rank pass counts
        sh.apply(regions, "render-prepare")
        self.rule.done("render", addr, regions["cnt"])
        return key + (True,)

    def render_backward(self, B, key, v1=False):
        regions, total = render_regions(B)
        addr, sh = self._ws("render", regions, total)
        fresh = key[:2] == (self.pack_gen, addr)
        self.pack_gen += 1
        if v1 or not key[2]:
            self.rule.spoil("render")
            sh.apply(regions, "render-backward-v1" if v1 else "render-backward")
            return
        if not fresh:
            self.rule.begin("render", addr, regions["cnt"])
            sh.zero(regions["cnt"])
        sh.apply(regions, "render-backward")
        if not fresh:
            self.rule.done("render", addr, regions["cnt"])


def drive(sim, op, descs, skip_backward=None, **kw):
    """Forward + backward per entry of `descs` ((B, C) for the lift, B for the render, B for the whole "step") on `sim`;
    the forward at index `skip_backward` is left without its backward.  Returns the Promise log's slice per entry."""
    cuts = []
    for i, desc in enumerate(descs):
        n = len(sim.log)
        if op == "lift":
            key = sim.lift_forward(*desc, **kw)
            if i != skip_backward:
                sim.lift_backward(*desc, key)
        elif op == "render":
            key = sim.render_forward(desc, **kw)
            if i != skip_backward:
                sim.render_backward(desc, key, v1=kw.get("path") == "v1")
        else:
            lkey = sim.lift_forward(desc, 4, cl=kw.get("cl", True))
            rkey = sim.render_forward(desc)
            if i != skip_backward:
                sim.render_backward(desc, rkey)
                sim.lift_backward(desc, 4, lkey)
        cuts.append(sim.log[n:])
    return cuts


def twice(seq):
    return [x for x in seq for _ in range(2)]


B_SEQS = [(2, 1, 2), (4, 1, 4), (3, 2, 3)]
LIFT_SEQS = [[(b, 4) for b in s] for s in B_SEQS] + [[(2, 8), (2, 4), (2, 8)]]


def sequences():
    """(name, op, descs, kw) of every plain sequence, each descriptor run twice in a row."""
    for seq in LIFT_SEQS:
        for cl in (False, True):
            for defer in (True, False):
                yield f"lift {seq} cl={cl} defer={defer}", "lift", twice(seq), dict(cl=cl, defer=defer)
    for seq in B_SEQS:
        for path in ("merged", "planned", "v1"):
            yield f"render {seq} {path}", "render", twice(list(seq)), dict(path=path)
        for cl in (False, True):
            yield f"step {seq} cl={cl}", "step", twice(list(seq)), dict(cl=cl)


def check_log(name, log):
    bad = [p for p in log if p.promised and not p.zero]
    assert not bad, f"{name}: a *_CLEAN promise over bytes that are not zero: {bad}"


# ---------------------------------------------------------------------------------------------------- CPU tests
def test_state_events():
    """CounterState by itself: fresh buffer, call in flight, pass completed for one range, call raised, new buffer."""
    s, r1, r2 = CounterState(), (1024, 512), (4096, 512)
    assert not s.begin("lift", 7, r1)                   # nothing known
    s.fresh("lift", 7)
    s.use("lift", 7, r1)
    assert s.begin("lift", 7, r1)                       # fresh: any range
    assert not s.begin("lift", 7, r1)                   # in flight (or raised): not clean
    s.done("lift", 7, r1)
    s.use("lift", 7, r1)
    assert s.begin("lift", 7, r1)
    s.done("lift", 7, r1)
    s.use("lift", 7, r2)                                # a call of another layout: void
    assert not s.begin("lift", 7, r2)
    s.done("lift", 7, r2)
    assert not s.begin("lift", 7, r1)                   # clean for r2 and for no other
    s.done("lift", 7, r1)
    assert not s.begin("lift", 8, r1)                   # another buffer
    s.fresh("lift", 9)
    s.done("lift", 7, r1)                               # a pass that ends on the replaced buffer says nothing of the new
    assert s.begin("lift", 9, r2)
    s.done("lift", 9, r2)
    s.spoil("lift")
    assert not s.begin("lift", 9, r2)
    s.fresh("lift", 9)
    s.use("lift", 9, r1)                                # a fresh buffer worked on by layout r1 ...
    assert not s.begin("lift", 9, r2)                   # ... is no longer known zero at r2
    s.fresh("render", 3)
    assert s.begin("render", 3, r1) and not s.begin("lift", 3, r1)       # keys are separate


def test_new_state_never_promises_over_dirty_bytes():
    """Every sequence, complete and with one forward left without its backward: a promise is made only where the
    shadow model has the counters zero, and IS made on the second and later calls of an unchanged descriptor."""
    n = 0
    for name, op, descs, kw in sequences():
        for skip in (None, 1, 2, 3):
            sim = Sim(CounterState())
            cuts = drive(sim, op, descs, skip_backward=skip, **kw)
            check_log(f"{name} skip={skip}", sim.log)
            if kw.get("path") == "v1":
                assert not sim.log                      # (no prepare pass in a v1 training forward: nothing to promise)
                continue
            for i, cut in enumerate(cuts):
                assert cut, (name, i)
                # the freshly allocated buffer, and every repeat of a descriptor (a skipped lift backward leaves its
                # forward's scan pending, which the next forward runs: still the same descriptor's range)
                if i == 0 or i % 2 == 1:
                    assert all(p.promised for p in cut), f"{name} skip={skip}: call {i} does not promise: {cut}"
                else:
                    # a changed descriptor, on the buffer the first (the largest) one allocated: never
                    assert not any(p.promised for p in cut), f"{name} skip={skip}: call {i} promises: {cut}"
            n += 1
    assert n > 100
    # a no-grad call at the other B between a forward and its backward
    for cl in (False, True):
        for path in ("merged", "planned"):
            sim = Sim(CounterState())
            drive(sim, "step", [2, 2], cl=cl)
            lkey, rkey = sim.lift_forward(2, 4, cl=cl), sim.render_forward(2, path=path)
            for b in (1, 4):
                sim.lift_forward(b, 4, grad=False, cl=cl)
                sim.render_forward(b, path=path, grad=False)
            sim.render_backward(2, rkey)
            sim.lift_backward(2, 4, lkey)
            cuts = drive(sim, "step", [2, 2], cl=cl)
            check_log(f"no-grad between cl={cl} {path}", sim.log)
            assert all(p.promised for p in cuts[1])
    # a call that raises between its first and last launch: in flight for good, until a pass completes
    for op, fwd, bwd, a in (("lift", Sim.lift_forward, Sim.lift_backward, (2, 4)), ("render", Sim.render_forward, Sim.render_backward, (2,))):
        for kw in ((dict(defer=False), dict(defer=True)) if op == "lift" else (dict(path="merged"), dict(path="planned"))):
            sim = Sim(CounterState())
            bwd(sim, *a, fwd(sim, *a, **kw))
            assert fwd(sim, *a, raises=True, **kw) is None
            assert sim.log[-1].promised                 # (it did promise, rightly; then it raised)
            n = len(sim.log)
            bwd(sim, *a, fwd(sim, *a, **kw))
            assert [p.promised for p in sim.log[n:]] == [False], sim.log[n:]
            bwd(sim, *a, fwd(sim, *a, **kw))
            assert sim.log[-1].promised
            check_log(f"{op} raises {kw}", sim.log)


# (sequence on one HotPath, the old layout, the new layout, the old regions under the new counters) -- as computed from
# the layout functions when the bookkeeping was fixed
HAZARDS = [
    ("lift", (1, 4), (2, 4), ["ptaps"]),
    ("lift", (2, 4), (3, 4), ["amask", "ptaps"]),
    ("lift", (2, 4), (2, 8), ["ptaps"]),
    ("lift", (2, 4), (1, 4), ["gfeat_cl"]),
    ("lift", (4, 4), (1, 4), ["feat_cl"]),
    ("lift", (1, 4), (4, 4), ["ptaps"]),
    ("render", 1, 4, ["rank"]),
    ("render", 1, 2, ["part"]),
    ("render", 1, 3, ["part"]),
    ("render", 2, 3, ["part"]),
    ("render", 2, 1, ["packed"]),
    ("render", 4, 1, ["packed"]),
    ("render", 3, 2, ["grad", "gcl"]),
]


def test_layouts_are_real_hazards():
    """Which region of the previous call's layout the new call's counters lie over, from the layout functions: the GPU
    sequences below move the counters onto bytes that calls write.  (fp32 and bf16 render descriptors: one layout.)"""
    for op, old, new, want in HAZARDS:
        if op == "lift":
            (ro, to), (rn, tn) = lift_regions(*old), lift_regions(*new)
        else:
            (ro, to), (rn, tn) = render_regions(old), render_regions(new)
            assert render_regions(new, bf16=True) == render_regions(new)
        assert under_cnt(rn, ro) == want, (op, old, new, under_cnt(rn, ro))
        assert ro["cnt"] != rn["cnt"]
    # every step of the GPU sequences that returns to the larger descriptor finds its counters over bytes that the
    # smaller one's TRAINING FORWARD writes (pair taps; drawn ranks), and the buffer is not replaced on the way
    written = set(WRITES["lift-emit"][0])
    for seq in LIFT_SEQS:
        small, big = seq[1], seq[0]
        assert lift_regions(*big)[1] > lift_regions(*small)[1]
        assert set(under_cnt(lift_regions(*big)[0], lift_regions(*small)[0])) & written, seq
    assert set(under_cnt(render_regions(4)[0], render_regions(1)[0])) & set(WRITES["render-merged-train"][0])
    for small, big in ((1, 2), (2, 3)):
        assert set(under_cnt(render_regions(big)[0], render_regions(small)[0])) & set(WRITES["render-backward"][0])


@pytest.mark.parametrize("op,seq,kw", [("lift", [(2, 4), (1, 4), (2, 4)], dict(cl=True)), ("lift", [(4, 4), (1, 4), (4, 4)], dict(cl=False)),
                                       ("render", [2, 1, 2], dict(path="merged")), ("render", [4, 1, 4], dict(path="merged")),
                                       ("step", [2, 1, 2], {}), ("step", [4, 1, 4], {})])
def test_parent_rule_promises_over_dirty_bytes(op, seq, kw):
    """The rule of the commit before, on the same model: at the return to the larger batch it promises *_CLEAN over
    bytes the smaller batch's calls have written.  (What the tests of this file detect.)"""
    sim = Sim(ParentRule())
    cuts = drive(sim, op, seq, **kw)
    assert all(p.promised and p.zero for p in cuts[0])                  # the fresh buffer: rightly
    assert any(p.promised and not p.zero for p in cuts[2]), cuts[2]
    with pytest.raises(AssertionError, match="promise over bytes that are not zero"):
        check_log("parent", sim.log)
    sim = Sim(CounterState())                                           # and the new state on the same calls
    cuts = drive(sim, op, seq, **kw)
    check_log("new", sim.log)
    assert not any(p.promised for p in cuts[2])


# ---------------------------------------------------------------------------------------------------- GPU: helpers
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def checks(dev):
    """vamp_debug_checks(1) for the test's duration: a broken promise is refused before the library relies on it."""
    lib = _capi.load()
    lib.vamp_debug_checks(1)
    try:
        yield lib
    finally:
        lib.vamp_debug_checks(0)
        torch.cuda.synchronize()


class Recorder(_Calls):
    """_Calls that records the lift entry points too, and raises a host exception in front of the calls named in
    `fail_at` (nothing is launched by a call that raises here)."""

    def __init__(self, lib, fail_at=()):
        super().__init__(lib)
        self.fail_at = set(fail_at)

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("vamp_render", "vamp_lift")):
            return fn

        def call(*a):
            if name in self.fail_at:
                raise RuntimeError(f"injected failure in front of {name}")
            self.log.append((name, a))
            return fn(*a)
        return call


# position of the flag word in the argument lists (include/vampire_hip.h)
FLAG_AT = {"vamp_lift_forward_ex": -2, "vamp_lift_backward_ex": -2, "vamp_render_forward_merged": -2,
           "vamp_render_camera_prepare_ex": -2, "vamp_render_camera_prepare_with_lift": 7,
           "vamp_render_camera_forward_ex": -2, "vamp_render_camera_backward_acc": -3, "vamp_render_bev_forward_ex": -2,
           "vamp_render_bev_backward_ex": -2}
PREPARES = ("vamp_render_camera_prepare_ex", "vamp_render_camera_prepare_with_lift")
CAM_VALID = (_capi.VAMP_CAMBWD_PACKED_VALID | _capi.VAMP_CAMBWD_CELLS_VALID | _capi.VAMP_CAMBWD_TERM_VALID
             | _capi.VAMP_CAMBWD_SAMPLES_VALID)


def flag_log(log):
    """[(entry point, flag word)] of the recorded calls that carry one."""
    return [(n, a[FLAG_AT[n]]) for n, a in log if n in FLAG_AT]


def lift_promises(log):
    return [bool(f & _capi.VAMP_LIFTFWD_CELLS_CLEAN) for n, f in flag_log(log)
            if n == "vamp_lift_forward_ex" and f & _capi.VAMP_LIFTFWD_EMIT_PAIRS]


def render_promises(log):
    """One per counting pass of a training forward: the merged launch that draws ranks, or a full prepare pass."""
    out = []
    for n, f in flag_log(log):
        if n == "vamp_render_forward_merged" and f & _capi.VAMP_RENDERFWD_RANK:
            out.append(bool(f & _capi.VAMP_RENDERFWD_COUNTERS_CLEAN))
        elif n in PREPARES and not f & _capi.VAMP_CAMPREP_RANKED:
            out.append(bool(f & _capi.VAMP_CAMPREP_COUNTERS_CLEAN))
        elif n in PREPARES:
            assert not f & _capi.VAMP_CAMPREP_COUNTERS_CLEAN, (n, f)   # (the ranked scan takes no promise)
    return out


@functools.lru_cache(maxsize=None)
def lift_seq_scene(B, C_):
    """test_render_shape_sweep.lift_scene at D = 21 with B samples and C_ channels (probabilities in)."""
    cfg = dataclasses.replace(CFG, mid_channels=C_)
    s2e, intrin, ida = synthetic.camera_rig(cfg, B, jitter=1.0, seed=5)
    lm = lift_matrices(s2e, intrin, ida, synthetic.bda_matrix(B, rot_deg=5.0))
    gen = torch.Generator().manual_seed(900 + 16 * B + C_)
    depth = (torch.randn(B, NCAM, cfg.D, cfg.fH, cfg.fW, generator=gen) * 2).softmax(dim=2)
    feat = torch.randn(B, NCAM, C_, cfg.fH, cfg.fW, generator=gen)
    feat[:, :, 1, ::3] = 0.0                     # exact zeros in a channel: the per-channel hit count (bv2:509-512)
    geo = PathGeometry(cfg)
    with torch.no_grad():                        # voxels whose only samples are exact zeros carry a 1e6 factor: no upstream there
        pix = O.ego_to_pixel(geo.voxel_coords, None, None, None, None, lm)
        valid, grid = O.lift_valid_and_grid(pix, cfg.final_dim, cfg.d_bound)
        sm = torch.nn.functional.grid_sample(O.outer_depth_feat(depth, feat).flatten(0, 1), grid.flatten(0, 1),
                                             align_corners=False)
        sm = sm.reshape(B, NCAM, C_, *grid.shape[2:5])
        fragile = ((sm.abs() < 1e-7) & valid.bool().unsqueeze(2)).any(dim=1)
    gout = torch.randn(B, C_, cfg.vZ, cfg.vY, cfg.vX, generator=gen)
    gout[fragile] = 0.0
    return cfg, geo, lm, depth, feat, gout


@functools.lru_cache(maxsize=None)
def lift_seq_oracle(B, C_):
    """float64 oracle lift of the scene: forward, grad depth, grad feat."""
    cfg, geo, lm, depth, feat, gout = lift_seq_scene(B, C_)
    d, f = depth.double().requires_grad_(True), feat.double().requires_grad_(True)
    out = O.lift(d, f, geo.voxel_coords, None, None, None, None, cfg.final_dim, cfg.d_bound, prepared=lm, compute_dtype=F64)
    out.backward(gout.double())
    return out.detach(), d.grad, f.grad


def channel_last(feat):
    """The same values in the memory of a torch.channels_last producer (vampire_amd.step.SyntheticBatch)."""
    return feat.permute(0, 1, 3, 4, 2).contiguous().permute(0, 1, 4, 2, 3)


def lift_step(hp, dev, B, C_, cl, tag, backward=True):
    """Forward (+ backward) of hp.lift on the (B, C_) scene: [(what, error, bar)] against the float64 oracle, and the
    pending graph when the backward is left to the caller."""
    cfg, geo, lm, depth, feat, gout = lift_seq_scene(B, C_)
    ref_out, ref_gd, ref_gf = lift_seq_oracle(B, C_)
    d = depth.to(dev).requires_grad_(True)
    f = feat.to(dev)
    f = (channel_last(f) if cl else f).requires_grad_(True)
    out = hp.lift(d, f, lm.to(dev))
    errs = [(f"{tag} forward", rel_err(out, ref_out), LIFT_BAR)]

    def finish():
        out.backward(gout.to(dev))
        return [(f"{tag} grad depth", rel_err(d.grad, ref_gd), LIFT_GRAD_BAR),
                (f"{tag} grad feat", rel_err(f.grad, ref_gf), LIFT_GRAD_BAR)]
    if backward:
        return errs + finish()
    return errs, finish


@dataclasses.dataclass(frozen=True)
class RCase(RS.Case):
    """The sweep's tiny case with a batch size (test_render_shape_sweep.scene reads `B`)."""
    B: int = 2


def render_step(hp, dev, B, tag, backward=True, grad=True):
    """Forward (+ backward) of hp.render on the B-sample scene of the sweep: [(what, error, bar)] against the float64
    oracle -- eight outputs, four volume gradients, grad_beta -- at the bars of test_render_shape_sweep.run_path."""
    case = RCase("tiny", B=B)
    cfg, rm, vols, beta_v = scene(case)
    ref_outs, ref_grads, ref_gbeta, gbeta_scale = oracle_render(case)
    lv = [v.to(dev).requires_grad_(grad) for v in vols]
    beta = torch.tensor(beta_v, device=dev, requires_grad=grad)
    if grad:
        outs = hp.render(*lv, beta, render_mats=rm.to(dev))
    else:
        with torch.no_grad():
            outs = hp.render(*lv, beta, render_mats=rm.to(dev))
    errs = []
    for nm, o, r in zip(NAMES, outs, ref_outs):
        bar = OUT_BAR + (3 * 1.2e-7 * cfg.d_bound[1] / max(float(r.abs().max()), 1e-30) if nm == "depth_preds" else 0.0)
        errs.append((f"{tag} {nm}", rel_err(o, r), bar))

    def finish():
        torch.autograd.backward(outs, _upstream([o.shape for o in outs], 4545, dev))
        return ([(f"{tag} grad_{k}", rel_err(v.grad, r), GRAD_BAR) for k, v, r in zip(VOLS, lv, ref_grads)]
                + [(f"{tag} grad_beta", abs(float(beta.grad) - ref_gbeta) / gbeta_scale, BETA_BAR)])
    if backward and grad:
        return errs + finish()
    return errs if not grad else (errs, finish)


def report(name, errs):
    for what, e, bar in errs:
        print(f"{name} {what}: {e:.3e} (bar {bar:.1e})")
    bad = [f"{what}: {e:.3e} > {bar:.1e}" for what, e, bar in errs if not e <= bar]
    assert not bad, f"{name}:\n" + "\n".join(bad)


def hot_recorded(dev, **impl):
    hp = hot(CFG, dev)
    hp.impl.update(impl)
    hp.lib = rec = Recorder(hp.lib)
    return hp, rec


# ---------------------------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("defer", [True, False], ids=["defer", "scan-in-call"])
@pytest.mark.parametrize("cl", [False, True], ids=["channel-first", "channel-last"])
@pytest.mark.parametrize("seq", [LIFT_SEQS[0], LIFT_SEQS[1], LIFT_SEQS[3]], ids=["B2-1-2", "B4-1-4", "C8-4-8"])
def test_lift_sequences(dev, checks, seq, cl, defer):
    """One HotPath, forward + backward per step (the last descriptor once more): every output and gradient against the
    oracle; CELLS_CLEAN on the fresh buffer's first call and on the repeated descriptor only, as the model says."""
    seq = seq + seq[-1:]
    hp, rec = hot_recorded(dev, lift_bwd="cell", defer_lift_scan=defer)
    errs = []
    for i, (B, C_) in enumerate(seq):
        errs += lift_step(hp, dev, B, C_, cl, f"step {i} B={B} C={C_}")
    torch.cuda.synchronize()
    sim = Sim(CounterState())
    drive(sim, "lift", seq, cl=cl, defer=defer)
    want = [p.promised for p in sim.log]
    assert want == [True, False, False, True]
    assert lift_promises(rec.log) == want, flag_log(rec.log)
    report(f"lift {seq} cl={cl} defer={defer}", errs)


RENDER_PATHS = {"merged": ("merged", "merged"), "planned-ert": ("planned-ert", "planned"),
                "planned-noert": ("planned-noert", "planned"), "v1": ("v1", "v1")}


@pytest.mark.gpu
@pytest.mark.parametrize("seq,path", [(s, p) for s in B_SEQS for p in ("merged", "planned-ert", "planned-noert")]
                         + [(B_SEQS[0], "v1")], ids=lambda v: str(v).replace(" ", ""))
def test_render_sequences(dev, checks, seq, path):
    """The same through hp.render on the merged path, the planned path with and without early termination, and (B = 2,
    1, 2) the v1 cross-check: eight outputs, four volume gradients and grad_beta per step against the oracle; the
    COUNTERS_CLEAN flags as the model says."""
    seq = list(seq) + [seq[-1]]
    impl, model_path = RENDER_PATHS[path]
    hp, rec = hot_recorded(dev, **PATHS[impl])
    errs = []
    for i, B in enumerate(seq):
        errs += render_step(hp, dev, B, f"step {i} B={B}")
    torch.cuda.synchronize()
    sim = Sim(CounterState())
    drive(sim, "render", seq, path=model_path)
    want = [p.promised for p in sim.log]
    assert want == ([] if path == "v1" else [True, False, False, True])
    assert render_promises(rec.log) == want, flag_log(rec.log)
    merged = [f for n, f in flag_log(rec.log) if n == "vamp_render_forward_merged"]
    assert (len(merged) == len(seq) and all(f & _capi.VAMP_RENDERFWD_RANK for f in merged)) == (path == "merged"), merged
    report(f"render {seq} {path}", errs)


@pytest.mark.gpu
@pytest.mark.parametrize("cl", [False, True], ids=["channel-first", "channel-last"])
def test_no_grad_call_between_forward_and_backward(dev, checks, cl):
    """Training forward at B = 2, a no-grad forward at B = 1 (lift, then render), then the B = 2 backward: it promises
    none of the forward's leavings and still gives every gradient; the next steps promise as the model says."""
    hp, rec = hot_recorded(dev, **PATHS["merged"])
    errs = lift_step(hp, dev, 2, 4, cl, "warm") + render_step(hp, dev, 2, "warm")
    le, lift_back = lift_step(hp, dev, 2, 4, cl, "train", backward=False)
    re_, render_back = render_step(hp, dev, 2, "train", backward=False)
    with torch.no_grad():
        cfg, geo, lm, depth, feat, gout = lift_seq_scene(1, 4)
        f1 = feat.to(dev)
        o1 = hp.lift(depth.to(dev), channel_last(f1) if cl else f1, lm.to(dev))
    errs.append(("no-grad lift B=1", rel_err(o1, lift_seq_oracle(1, 4)[0]), LIFT_BAR))
    errs += render_step(hp, dev, 1, "no-grad B=1", grad=False)
    n = len(rec.log)
    errs += le + re_ + render_back() + lift_back()
    back = flag_log(rec.log[n:])
    cam = [f for nm, f in back if nm == "vamp_render_camera_backward_acc"]
    lift = [f for nm, f in back if nm == "vamp_lift_backward_ex"]
    assert cam and not any(f & CAM_VALID for f in cam), cam
    assert len(lift) == 1 and not lift[0] & _capi.VAMP_LIFTBWD_CELLS_VALID, lift
    n = len(rec.log)
    for i in range(2):
        errs += lift_step(hp, dev, 2, 4, cl, f"after {i}") + render_step(hp, dev, 2, f"after {i}")
    torch.cuda.synchronize()
    # (the backwards re-listed on their own layouts: B = 2's counters are zero again, and known to be)
    assert lift_promises(rec.log[n:]) == [True, True] and render_promises(rec.log[n:]) == [True, True], flag_log(rec.log[n:])
    report(f"no-grad between cl={cl}", errs)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["merged", "planned-ert"])
def test_call_that_raises_at_the_prepare_pass(dev, checks, path):
    """A host exception in front of the prepare pass of a render forward (the counters counted, not scanned): the next
    step sends no *_CLEAN promise, passes the debug checks and matches the oracle; the step after promises again."""
    hp, rec = hot_recorded(dev, **PATHS[path])
    errs = render_step(hp, dev, 2, "step 0")
    rec.fail_at = set(PREPARES)
    with pytest.raises(RuntimeError, match="injected failure"):
        render_step(hp, dev, 2, "raises")
    rec.fail_at = set()
    torch.cuda.synchronize()
    n = len(rec.log)
    errs += render_step(hp, dev, 2, "step 2")
    assert render_promises(rec.log[n:]) == [False], flag_log(rec.log[n:])
    n = len(rec.log)
    errs += render_step(hp, dev, 2, "step 3")
    torch.cuda.synchronize()
    assert render_promises(rec.log[n:]) == [True], flag_log(rec.log[n:])
    report(f"raise at prepare {path}", errs)


def whole_step(model, batch):
    """train_step: (vox, eight outputs, grad depth, grad feat, four volume gradients, grad beta), cloned."""
    from vampire_amd.step import train_step
    model.zero_grad(set_to_none=True)
    vox, outs = train_step(model, batch)
    got = [vox] + list(outs) + [batch.depth.grad, batch.feat.grad] + [v.grad for v in batch.vols] + [model.beta.grad]
    return [t.detach().clone() for t in got]


STEP_WHAT = ["lift"] + NAMES + ["grad_depth", "grad_feat"] + ["grad_" + v for v in VOLS] + ["grad_beta"]
STEP_BARS = [LIFT_BAR] + [OUT_BAR] * 8 + [LIFT_GRAD_BAR] * 2 + [GRAD_BAR] * 4 + [BETA_BAR]


@pytest.mark.gpu
@pytest.mark.parametrize("cl", [True, False], ids=["channel-last", "channel-first"])
def test_whole_step_across_batch_sizes(dev, checks, cl):
    """LiftRenderStep + SyntheticBatch + train_step at B = 2, 2, 1, 2, 2 on ONE model: every step's outputs and input
    gradients equal those of a fresh model given the same batch, within the sweep's bars relative to the fresh model's
    values; the flags of every C call of the last step equal those of the first steady-state step (the second), and
    the forwards right behind the detour differ from them by the *_CLEAN promises alone."""
    from vampire_amd.step import LiftRenderStep, SyntheticBatch
    batches = {B: SyntheticBatch(CFG, B, dev, seed=3, feat_channel_last=cl) for B in (2, 1)}
    ref = {B: whole_step(LiftRenderStep(CFG, dev), b) for B, b in batches.items()}
    model = LiftRenderStep(CFG, dev)
    model.hp.lib = rec = Recorder(model.hp.lib)
    errs, flags = [], []
    for i, B in enumerate((2, 2, 1, 2, 2)):
        n = len(rec.log)
        got = whole_step(model, batches[B])
        flags.append(flag_log(rec.log[n:]))
        errs += [(f"step {i} B={B} {w}", rel_err(a, b), bar) for w, a, b, bar in zip(STEP_WHAT, got, ref[B], STEP_BARS)]
    torch.cuda.synchronize()
    assert flags[4] == flags[1], (flags[1], flags[4])
    assert any(f & _capi.VAMP_LIFTFWD_CELLS_CLEAN for n, f in flags[1] if n == "vamp_lift_forward_ex")
    assert any(f & _capi.VAMP_RENDERFWD_COUNTERS_CLEAN for n, f in flags[1] if n == "vamp_render_forward_merged")
    clean = {"vamp_lift_forward_ex": _capi.VAMP_LIFTFWD_CELLS_CLEAN, "vamp_render_forward_merged": _capi.VAMP_RENDERFWD_COUNTERS_CLEAN}
    # (the BEV backward's TABLE_VALID follows B too -- _bev_tab_key -- and is not this file's subject)
    assert ([(n, f) for n, f in flags[3] if n in clean]
            == [(n, f & ~clean[n]) for n, f in flags[1] if n in clean]), (flags[1], flags[3])
    sim = Sim(CounterState())
    drive(sim, "step", [2, 2, 1, 2, 2], cl=cl)
    assert lift_promises(rec.log) == [p.promised for p in sim.log if p.op == "lift"] == [True, True, False, False, True]
    assert render_promises(rec.log) == [p.promised for p in sim.log if p.op == "render"] == [True, True, False, False, True]
    report(f"whole step cl={cl}", errs)


@pytest.mark.gpu
def test_merged_launch_checks_every_counter(dev, checks):
    """vamp_debug_checks(1) on the merged training launch covers all ncell + 64 counters: one counter past index 64
    non-zero under VAMP_RENDERFWD_COUNTERS_CLEAN is refused before the launch."""
    hp, rec = hot_recorded(dev, **PATHS["merged"])
    errs = render_step(hp, dev, 2, "step 0")
    torch.cuda.synchronize()
    ws = hp._ws["render"]
    off, nbytes = render_regions(2)[0]["cnt"]
    cnt = ws[off:off + nbytes].view(torch.int32)
    assert int(cnt.abs().max()) == 0 and cnt.numel() > 1000
    cnt[1000] = 1
    hp._counters.fresh("render", ws.data_ptr())
    with pytest.raises(_capi.VampireHipError, match="promise broken.*COUNTERS_CLEAN"):
        render_step(hp, dev, 2, "refused")
    assert [n for n, _ in rec.log].count("vamp_render_forward_merged") == 2      # (the refused call was the merged launch)
    ws.zero_()
    hp._counters.fresh("render", ws.data_ptr())
    errs += render_step(hp, dev, 2, "step 2")
    torch.cuda.synchronize()
    report("widened check", errs)
