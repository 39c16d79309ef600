"""CPU checks of the render's schedule tables (vampire_amd.ops.render_forward_plan, render_backward_plan): every
combination of their inputs gives a well-formed list of calls, and the backward's calls carry exactly the promises
(`*_VALID`) and the overwrite / accumulate roles the library's contract allows."""
import itertools

from vampire_amd import _capi
from vampire_amd.ops import render_backward_plan, render_forward_plan

F = _capi


def test_merged_schedules():
    """The one-launch render forward stands for "cam" + "bev": exactly where the one-kernel camera forward with early
    termination runs forward-only, never otherwise."""
    for train, two, prep_ok, direct, ert in itertools.product((False, True), repeat=5):
        plan = render_forward_plan(train, two, prep_ok, direct, ert, merged=True)
        ops = [p[0] for p in plan]
        if direct and ert and not train:
            assert ops == ["render"] and plan[0][1] == "cur" and plan[0][2] == 0, ((train, two, prep_ok, direct, ert), ops)
        elif direct and ert and train and prep_ok:
            # training: the one launch also draws the backward's cell ranks; scan + heavy list behind it
            assert ops == ["render", "prep"] and plan[0][1] == "cur" and plan[0][2] == _capi.VAMP_RENDERFWD_RANK
            assert plan[1][2] == _capi.VAMP_CAMPREP_RANKED and plan[1][1] == "cur"
        else:
            assert plan == render_forward_plan(train, two, prep_ok, direct, ert), (train, two, prep_ok, direct, ert)


def test_every_schedule_is_well_formed():
    for train, two, prep_ok, direct, ert in itertools.product((False, True), repeat=5):
        plan = render_forward_plan(train, two, prep_ok, direct, ert)
        ops = [p[0] for p in plan]
        key = (train, two, prep_ok, direct, ert)
        assert ops.count("bev") == 1 and ops.count("cam") == 1, (key, ops)
        recorded = set()
        for op, where, flags, waits, records in plan:
            assert where in ("cur", "side") and (two or where == "cur"), (key, op, where)
            assert set(waits) <= recorded, (key, op, waits)          # an event is recorded before it is waited for
            recorded |= set(records)
        cam = next(p for p in plan if p[0] == "cam")
        assert cam[1] == "cur"                                       # the outputs appear on the caller's stream
        assert bool(cam[2] & _capi.VAMP_CAMFWD_DIRECT) == direct, key
        # a termination pre-pass exactly when the planned march runs with early termination, and then the march
        # (and the prepare pass) are told the table is there and wait for it
        assert ("term" in ops) == (ert and not direct), key
        assert bool(cam[2] & _capi.VAMP_CAMFWD_TERM_VALID) == ("term" in ops), key
        if "pack" in ops:
            assert cam[2] & _capi.VAMP_CAMFWD_PACKED_VALID and "packed" in cam[3], key
            assert ops.index("term") < ops.index("pack") < ops.index("cam"), key
        # the prepare pass only in front of the cell-list backward of a two-stream training step
        assert ("prep" in ops) == (train and two and prep_ok), key
        if "prep" in ops:
            prep = next(p for p in plan if p[0] == "prep")
            assert prep[1] == "side"
            has_table = direct or ert
            assert bool(prep[2] & _capi.VAMP_CAMPREP_TERM_VALID) == has_table, key
            if has_table:       # the table's producer is ahead of it: on its own stream, or through an event
                src = "cam" if direct else "term"
                producer = next(p for p in plan if p[0] == src)
                assert ops.index(src) < ops.index("prep") and (producer[1] == "side" or set(prep[3]) & set(producer[4])), key


# ---------------------------------------------------------------------------------------------------- the backward
BWD_INPUTS = ("two", "matrices", "cell_impl", "fresh", "cells", "samples", "ert", "packed", "bev_cell", "bev_saved",
              "tab_valid")
CAM_PARTS = F.VAMP_CAMBWD_PART_RAY | F.VAMP_CAMBWD_PART_HEAVY | F.VAMP_CAMBWD_PART_GATHER
BEV_PARTS = F.VAMP_BEVBWD_SKIP_BASE | F.VAMP_BEVBWD_ONLY_BASE
BEV_OVERWRITES = F.VAMP_BEVBWD_OVERWRITE_BASE | F.VAMP_BEVBWD_OVERWRITE_CAM


def backward_plans():
    for values in itertools.product((False, True), repeat=len(BWD_INPUTS)):
        k = dict(zip(BWD_INPUTS, values))
        yield k, render_backward_plan(**k)


def ordered(plan, i, j):
    """Call i of the plan is complete before call j starts: issued earlier on the same stream, or an event recorded on
    i's stream at or behind call i is waited for on j's stream at or in front of call j."""
    if not i < j:
        return False
    if plan[i][1] == plan[j][1]:
        return True
    events = {r for k in range(i, j) if plan[k][1] == plan[i][1] for r in plan[k][4]}
    return any(plan[m][1] == plan[j][1] and events & set(plan[m][3]) for m in range(i + 1, j + 1))


def test_backward_streams_and_events():
    for k, plan in backward_plans():
        assert {p[0] for p in plan} == {"cam", "bev"}, (k, plan)
        recorded = {}
        for op, where, flags, waits, records in plan:
            assert where in ("cur", "side") and (k["two"] or where == "cur"), (k, op, where)
            for w in waits:                 # every waited event is recorded earlier, on the other stream
                assert w in recorded and recorded[w] != where, (k, op, w)
            # only the camera call waits (the executor hands its event to the library), and for one event at most
            assert not waits or (op == "cam" and len(waits) == 1), (k, op, waits)
            recorded.update({r: where for r in records})
        assert [p for p in plan if p[0] == "cam"][-1][1] == "cur", k        # the gradients appear on the caller's stream


def test_backward_parts():
    """One camera call without part flags, or two with disjoint parts that cover all three, the gather last; one BEV
    call without part flags, or SKIP_BASE then ONLY_BASE on one stream with equal OVERWRITE flags."""
    for k, plan in backward_plans():
        cam = [p for p in plan if p[0] == "cam"]
        bev = [p for p in plan if p[0] == "bev"]
        if len(cam) == 1:
            assert not (cam[0][2] & CAM_PARTS), (k, cam)
        else:
            (a, b) = [p[2] & CAM_PARTS for p in cam]
            assert len(cam) == 2 and not (a & b) and (a | b) == CAM_PARTS and b == F.VAMP_CAMBWD_PART_GATHER, (k, cam)
            assert cam[0][2] & ~CAM_PARTS == cam[1][2] & ~CAM_PARTS, (k, cam)      # same VALID / ACCUMULATE flags
        if len(bev) == 1:
            assert not (bev[0][2] & BEV_PARTS), (k, bev)
        else:
            assert [p[2] & BEV_PARTS for p in bev] == [F.VAMP_BEVBWD_SKIP_BASE, F.VAMP_BEVBWD_ONLY_BASE], (k, bev)
            assert bev[0][1] == bev[1][1] and bev[0][2] & BEV_OVERWRITES == bev[1][2] & BEV_OVERWRITES, (k, bev)
            assert bev[0][2] & ~BEV_PARTS == bev[1][2] & ~BEV_PARTS, (k, bev)
        assert all(p[2] & F.VAMP_BEVBWD_OVERWRITE_BASE for p in bev), (k, bev)


def test_backward_first_writer_overwrites_and_the_second_accumulates():
    """grad_density_feature, grad_semantic and grad_rgb are written by the camera gather and by the BEV call that is
    not the ONLY_BASE half: exactly one of the two overwrites, and it is complete before the other starts."""
    for k, plan in backward_plans():
        gather = max(i for i, p in enumerate(plan) if p[0] == "cam")
        bevs = [i for i, p in enumerate(plan) if p[0] == "bev"]
        bev_w = next(i for i in bevs if not (plan[i][2] & F.VAMP_BEVBWD_ONLY_BASE))
        accumulate = bool(plan[gather][2] & F.VAMP_CAMBWD_ACCUMULATE)
        assert accumulate == any(plan[i][2] & F.VAMP_BEVBWD_OVERWRITE_CAM and ordered(plan, i, gather) for i in bevs), \
            (k, plan)
        for i in bevs:
            assert (not plan[i][2] & F.VAMP_BEVBWD_OVERWRITE_CAM) == ordered(plan, gather, i), (k, plan)
        overwriters = [i for i in (gather, bev_w) if (i == gather and not accumulate)
                       or (i == bev_w and plan[i][2] & F.VAMP_BEVBWD_OVERWRITE_CAM)]
        assert len(overwriters) == 1, (k, plan)
        other = bev_w if overwriters[0] == gather else gather
        assert ordered(plan, overwriters[0], other), (k, plan)


def test_backward_promises():
    """Every validity flag is set exactly when its rule (`want`: the forward left the thing, and the workspace is fresh)
    says, on every call of its kind, and the library's preconditions hold on every camera call."""
    for k, plan in backward_plans():
        fresh = k["fresh"]
        want = {F.VAMP_CAMBWD_PACKED_VALID: fresh and k["packed"],
                F.VAMP_CAMBWD_CELLS_VALID: fresh and k["cells"],
                F.VAMP_CAMBWD_SAMPLES_VALID: fresh and k["samples"] and k["cell_impl"],
                F.VAMP_CAMBWD_TERM_VALID: fresh and k["ert"],
                F.VAMP_CAMBWD_NO_ERT: not k["ert"],
                F.VAMP_CAMBWD_SPLAT: not k["cell_impl"]}
        for op, where, flags, waits, records in plan:
            if op == "cam":
                for bit, on in want.items():
                    assert bool(flags & bit) == on, (k, hex(flags), hex(bit))
                if flags & F.VAMP_CAMBWD_CELLS_VALID and not flags & F.VAMP_CAMBWD_NO_ERT:
                    assert flags & F.VAMP_CAMBWD_TERM_VALID, (k, hex(flags))
                if flags & F.VAMP_CAMBWD_SPLAT:
                    assert not flags & F.VAMP_CAMBWD_ACCUMULATE and not waits, (k, hex(flags))
                if flags & F.VAMP_CAMBWD_ACCUMULATE or waits:
                    assert k["matrices"] and k["cell_impl"], (k, hex(flags))
                known = CAM_PARTS | F.VAMP_CAMBWD_ACCUMULATE
                assert not flags & ~(known | sum(want)), (k, hex(flags))
            else:
                # (the v1 BEV splat keeps nothing in the workspace: bev_cell gates both promises, inside the plan)
                assert bool(flags & F.VAMP_BEVBWD_SAVED_VALID) == (k["bev_saved"] and k["bev_cell"]), (k, hex(flags))
                if flags & F.VAMP_BEVBWD_TABLE_VALID:
                    assert flags & BEV_PARTS and k["tab_valid"] and k["bev_cell"], (k, hex(flags))
                if flags & BEV_PARTS:
                    assert bool(flags & F.VAMP_BEVBWD_TABLE_VALID) == (k["tab_valid"] and k["bev_cell"]), (k, hex(flags))
                assert not flags & ~(BEV_PARTS | BEV_OVERWRITES | F.VAMP_BEVBWD_SAVED_VALID
                                     | F.VAMP_BEVBWD_TABLE_VALID), (k, hex(flags))


def test_the_three_backward_schedules():
    """The schedules at the default configuration (merged training forward with early termination, cell-list
    backwards, the forward's workspaces untouched, the axis tables of an earlier step in place)."""
    default = dict(two=True, matrices=True, cell_impl=True, fresh=True, cells=True, samples=True, ert=True, packed=False,
                   bev_cell=True, bev_saved=True, tab_valid=True)
    valid = F.VAMP_CAMBWD_CELLS_VALID | F.VAMP_CAMBWD_SAMPLES_VALID | F.VAMP_CAMBWD_TERM_VALID
    cam = F.VAMP_CAMBWD_ACCUMULATE | valid
    bev = F.VAMP_BEVBWD_OVERWRITE_BASE | F.VAMP_BEVBWD_OVERWRITE_CAM | F.VAMP_BEVBWD_SAVED_VALID
    # two streams: both backwards in parts, the camera gather behind the BEV event
    assert render_backward_plan(**default) == [
        ("cam", "cur", cam | F.VAMP_CAMBWD_PART_RAY | F.VAMP_CAMBWD_PART_HEAVY, (), ()),
        ("bev", "side", bev | F.VAMP_BEVBWD_TABLE_VALID | F.VAMP_BEVBWD_SKIP_BASE, (), ("bev",)),
        ("bev", "side", bev | F.VAMP_BEVBWD_TABLE_VALID | F.VAMP_BEVBWD_ONLY_BASE, (), ()),
        ("cam", "cur", cam | F.VAMP_CAMBWD_PART_GATHER, ("bev",), ())]
    # one stream (impl["overlap"] off): the BEV backward overwrites, the camera backward adds
    assert render_backward_plan(**dict(default, two=False)) == [
        ("bev", "cur", bev, (), ()),
        ("cam", "cur", cam, (), ())]
    # explicit geometry (its forward: planned march without early termination, no cell lists, no sample rows): the
    # camera backward overwrites, the BEV backward adds to the three shared buffers
    geom = dict(default, matrices=False, cells=False, samples=False, ert=False, packed=True)
    assert render_backward_plan(**geom) == [
        ("cam", "cur", F.VAMP_CAMBWD_NO_ERT | F.VAMP_CAMBWD_PACKED_VALID, (), ()),
        ("bev", "cur", F.VAMP_BEVBWD_OVERWRITE_BASE | F.VAMP_BEVBWD_SAVED_VALID, (), ())]
    # ... and the same order for the v1 camera splat on matrices
    v1 = dict(default, cell_impl=False, cells=False, samples=False)
    assert render_backward_plan(**v1) == [
        ("cam", "cur", F.VAMP_CAMBWD_TERM_VALID | F.VAMP_CAMBWD_SPLAT, (), ()),
        ("bev", "cur", F.VAMP_BEVBWD_OVERWRITE_BASE | F.VAMP_BEVBWD_SAVED_VALID, (), ())]
