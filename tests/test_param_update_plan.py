"""CPU-side checks of the parameter update (vampire_amd/optim.py, vamp_param_update_*): the chunk plan is a pure
function of the tensor sizes that covers every element once, the C ABI refuses bad arguments before it touches a GPU,
and the Python host refuses CPU modules (there is no fallback)."""
import ctypes as C

import numpy as np
import pytest
import torch

from vampire_amd import _capi, optim
from vampire_amd.build import build_library

CH = optim.UPDATE_CHUNK
EDGE_SIZES = [1, 3, CH - 1, CH, CH + 1, 2 * CH + 3]
SMALL_SIZES = [1 + i % 7 for i in range(70)]


@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


def _check_plan(numels, kinds, chunk):
    pl = optim.plan_update(numels, kinds, chunk)
    n_chunks = len(pl.tensor)
    assert n_chunks == pl.n_param_chunks + pl.n_buffer_chunks
    assert all(len(a) == n_chunks for a in (pl.offset, pl.length, pl.state_offset, pl.kind))
    # every element of every tensor in exactly one chunk, no chunk across a tensor's end
    hits = [np.zeros(n, dtype=np.int32) for n in numels]
    state_hits = np.zeros(pl.total_state, dtype=np.int32)
    for t, o, n, s, k in zip(pl.tensor.tolist(), pl.offset.tolist(), pl.length.tolist(), pl.state_offset.tolist(),
                             pl.kind.tolist()):
        assert 1 <= n <= chunk and 0 <= o and o + n <= numels[t], (t, o, n)
        assert k == kinds[t]
        assert s == pl.tensor_state_offset[t] + o and s % 4 == 0          # the state side is 16-byte aligned
        hits[t][o:o + n] += 1
        state_hits[s:s + n] += 1
    assert all((h == 1).all() for h in hits)
    assert state_hits.max() <= 1 and int(state_hits.sum()) == sum(numels)   # no two tensors share a state element
    assert (pl.tensor_state_offset % 4 == 0).all() and pl.param_state % 4 == 0 and pl.total_state % 4 == 0
    # parameter chunks first, their state inside [0, param_state): exp_avg / exp_avg_sq need no more
    assert (pl.kind[:pl.n_param_chunks] == optim.KIND_PARAM).all()
    assert (pl.kind[pl.n_param_chunks:] == optim.KIND_EMA_ONLY).all()
    ends = pl.state_offset + pl.length
    assert (ends[:pl.n_param_chunks] <= pl.param_state).all() and (pl.state_offset[pl.n_param_chunks:] >= pl.param_state).all()
    # the chunk count is a function of the sizes alone
    assert n_chunks == sum(-(-n // chunk) for n in numels)
    assert pl.n_param_chunks == sum(-(-n // chunk) for n, k in zip(numels, kinds) if k == optim.KIND_PARAM)
    return pl


@pytest.mark.parametrize("kinds", ["params", "mixed"])
def test_plan_covers_the_edge_sizes_once(kinds):
    ks = [optim.KIND_PARAM] * len(EDGE_SIZES) if kinds == "params" else [i % 2 for i in range(len(EDGE_SIZES))]
    pl = _check_plan(EDGE_SIZES, ks, CH)
    per_tensor = np.bincount(pl.tensor, minlength=len(EDGE_SIZES)).tolist()
    assert sorted(per_tensor) == sorted([1, 1, 1, 1, 2, 3])


def test_plan_covers_seventy_tiny_tensors():
    pl = _check_plan(SMALL_SIZES, [optim.KIND_PARAM] * 50 + [optim.KIND_EMA_ONLY] * 20, CH)
    assert len(pl.tensor) == 70 and pl.n_param_chunks == 50
    assert pl.total_state == sum(-(-n // 4) * 4 for n in SMALL_SIZES)


def test_plan_is_a_pure_function_of_the_sizes():
    a = optim.plan_update(EDGE_SIZES + SMALL_SIZES, [0] * 76, CH)
    b = optim.plan_update(tuple(EDGE_SIZES + SMALL_SIZES), [0] * 76, CH)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    small = _check_plan(EDGE_SIZES + [0, 17], [0] * 8, 8)                  # another chunk size, an empty tensor
    assert len(small.tensor) == sum(-(-n // 8) for n in EDGE_SIZES + [17])
    with pytest.raises(ValueError):
        optim.plan_update([4], [0, 0])
    with pytest.raises(ValueError):
        optim.plan_update([4], [0], chunk=6)
    with pytest.raises(ValueError):
        optim.plan_update([4], [2])


def test_table_record_matches_the_header_struct():
    assert optim.CHUNK_DTYPE.itemsize == C.sizeof(_capi.VampUpdateChunk) == 32
    for name, _ in _capi.VampUpdateChunk._fields_:
        assert optim.CHUNK_DTYPE.fields[name][1] == getattr(_capi.VampUpdateChunk, name).offset
    assert C.sizeof(_capi.VampUpdateScalars) == 128 and C.sizeof(_capi.VampParamUpdateDesc) == 64
    for name, word in optim._W.items():
        assert getattr(_capi.VampUpdateScalars, name).offset == 4 * word, name
    assert optim.UPDATE_CHUNK == _capi.VAMP_UPDATE_CHUNK == 4096 and optim.UPDATE_CHUNK % 1024 == 0


def _desc(**kw):
    d = _capi.VampParamUpdateDesc(0.9, 0.999, 1e-8, 1e-7, 35.0, 0.999, 3, 2, _capi.VAMP_UPDATE_SCALE_DYNAMIC, 0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_abi_rejects_bad_arguments_without_gpu(lib):
    """Every refusal comes before any launch: the fake addresses are never dereferenced."""
    fake = 1 << 20                                   # non-NULL, aligned, never read
    need = lib.vamp_param_update_workspace_bytes(C.byref(_desc()))
    assert need >= 3 * 8

    def step(d, table=fake, m=fake, v=fake, ema=fake, sc=fake, ws=fake, wb=None):
        return lib.vamp_param_update_step(C.byref(d) if d is not None else None, table, m, v, ema, sc, ws,
                                          need if wb is None else wb, None)

    assert step(None) == -1 and lib.vamp_param_update_workspace_bytes(None) == 0
    assert step(_desc(), table=None) == -1 and b"table is NULL" in lib.vamp_last_error()
    assert step(_desc(n_param_chunks=0, n_buffer_chunks=0)) == -1 and b"no chunks" in lib.vamp_last_error()
    assert lib.vamp_param_update_workspace_bytes(C.byref(_desc(n_param_chunks=0, n_buffer_chunks=0))) == 0
    assert step(_desc(n_param_chunks=-1)) == -1
    for name in ("beta1", "beta2"):
        for bad in (1.0, -0.1, 1.5, float("nan")):
            assert step(_desc(**{name: bad})) == -1 and name.encode() in lib.vamp_last_error(), (name, bad)
            assert lib.vamp_param_update_workspace_bytes(C.byref(_desc(**{name: bad}))) == 0
    assert step(_desc(), wb=need - 1) == -2 and b"workspace" in lib.vamp_last_error()
    assert step(_desc(), ws=None) == -2
    assert step(_desc(), sc=None) == -1 and step(_desc(), m=None) == -1 and step(_desc(), v=None) == -1
    assert step(_desc(), ema=None) == -1 and b"ema" in lib.vamp_last_error()
    assert step(_desc(eps=-1.0)) == -1 and step(_desc(weight_decay=-1.0)) == -1 and step(_desc(ema_decay=1.0)) == -1
    assert step(_desc(scale_mode=3)) == -1 and step(_desc(reserved=1)) == -1
    assert step(_desc(), m=fake + 4) == -1 and b"16-byte aligned" in lib.vamp_last_error()


def test_cpu_modules_and_other_dtypes_are_refused():
    with pytest.raises(_capi.VampireHipError):
        optim.ParamUpdate(torch.nn.Linear(3, 2), lr=1e-3)
    with pytest.raises(ValueError):
        optim.ParamUpdate(torch.nn.ReLU(), lr=1e-3)
