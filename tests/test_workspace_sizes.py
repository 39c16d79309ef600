"""The workspace sizes and layouts are part of what a caller allocates by: every `*_bytes` entry point and both
`*_workspace_layout` entry points must keep returning, value for value, what tests/golden/workspace_sizes.json
records (tests/golden/make_workspace_sizes.py wrote it; the cases and their descriptors are in the fixture itself).
Host computations only: no GPU."""
import ctypes as C
import json
import os

import pytest

from vampire_amd import _capi, _header
from vampire_amd.build import build_library

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")

# the entry points that return a status and fill a structure, and that structure
LAYOUTS = {"vamp_lift_workspace_layout": "VampLiftWorkspaceLayout",
           "vamp_render_workspace_layout": "VampRenderWorkspaceLayout"}


def size_entry_points():
    """Every entry point the fixture has to cover: whatever the header declares as returning size_t, and the layouts."""
    protos = _header.read().prototypes
    return sorted([n for n, (ret, _) in protos.items() if ret == "size_t"] + list(LAYOUTS))


def to_struct(name, fields):
    """{"field": number | [numbers] | {nested fields} | [{nested fields}]} -> the ctypes structure `name`."""
    s = getattr(_capi, name)()
    types = dict(s._fields_)
    for f, v in fields.items():
        t = types[f]
        if isinstance(v, dict):
            setattr(s, f, to_struct(t.__name__, v))
        elif isinstance(v, list):
            for i, x in enumerate(v):
                getattr(s, f)[i] = to_struct(t._type_.__name__, x) if isinstance(x, dict) else x
        else:
            setattr(s, f, v)
    return s


def from_struct(s):
    """The reverse, every field (pointers, which no size depends on, left out)."""
    out = {}
    for f, t in s._fields_:
        v = getattr(s, f)
        if isinstance(v, C.Array):
            out[f] = [from_struct(x) if isinstance(x, C.Structure) else x for x in v]
        elif isinstance(v, C.Structure):
            out[f] = from_struct(v)
        elif t is not C.c_void_p:
            out[f] = v
    return out


def call(lib, fn, args):
    """One case: `args` as the fixture holds them, an integer or {"struct": name, "fields": {...}} each."""
    a = [to_struct(x["struct"], x["fields"]) if isinstance(x, dict) else x for x in args]
    if fn in LAYOUTS:
        out = getattr(_capi, LAYOUTS[fn])()
        status = getattr(lib, fn)(*a, C.byref(out))
        return {"status": status, "layout": from_struct(out)}
    return getattr(lib, fn)(*a)


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


@pytest.fixture(scope="module")
def cases():
    with open(FIXTURE) as f:
        return json.load(f)["cases"]


def test_fixture_covers_every_size_entry_point(cases):
    by_fn = {}
    for c in cases:
        by_fn.setdefault(c["fn"], set()).add(c["case"])
    assert sorted(by_fn) == size_entry_points()
    for fn, kinds in by_fn.items():
        assert {"smallest", "odd", "bench"} <= kinds, fn


def test_sizes_and_layouts_are_what_they_were(lib, cases):
    for c in cases:
        got = call(lib, c["fn"], c["args"])
        assert got == c["want"], f'{c["fn"]} [{c["case"]}]: {got} != {c["want"]}'
        if c["fn"] in LAYOUTS:
            assert got["status"] == 0
        elif c["fn"] != "vamp_resize2d_workspace_bytes":         # (needs none: 0 for every shape)
            assert got > 0, f'{c["fn"]} [{c["case"]}] refuses its descriptor'
