"""Camera images on the device (images.camera_images over the HIP kernels of camera_images.hip): Pillow's resize,
crop, flip and rotate as the reference loader's img_transform applies them, then the normalisation.

Two references.  tests/golden/camera_images.npz holds images and ida matrices made by the reference's own
img_transform with Pillow (make_camera_images_golden.py; the Pillow version is in the file).  `apply_plan` below
applies the int32 tables of an ImagePlan in numpy, from rules 1 - 4 of include/vampire_hip.h.  A CPU test holds it to
every byte of the fixture; that is what licenses using it in the GPU sweeps.  The normalisation (rule 5) restates
mmcv.imnormalize and is checked against its numpy fp32 statement only: its parity with OpenCV is unpinned.

Exactness: the images are integers and the normalisation is two fp32 operations, each rounded once, so every
comparison is torch.equal (floats as bit patterns)."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vampire_amd import _capi                                 # noqa: E402
from vampire_amd import images as I                           # noqa: E402
from vampire_amd.build import build_library                   # noqa: E402
from vampire_amd.config import CFG_TINY                       # noqa: E402

f32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_images.npz")
CASES = ("a", "b", "c")
MEAN, STD = I.IMG_MEAN, I.IMG_STD


def raw_frames(B, N, h, w):
    """The integer formula of make_camera_images_golden.py: [B, N, h, w, 3] uint8, saturated blocks with hashed
    texture in every third 16 x 8 region."""
    b, n, y, x, c = np.ogrid[:B, :N, :h, :w, :3]
    b, n, y, x, c = (v.astype(np.int64) for v in (b, n, y, x, c))
    block = ((x // 5 + y // 3 + n + b) % 2) * 255 + 0 * c
    tex = ((x * 7 + y * 13 + c * 31 + n * 5 + b * 3 + 1) * 2654435761 % 4294967296) >> 24
    return np.where((x // 16 + y // 8 + n) % 3 == 0, tex, block).astype(np.uint8)


def apply_plan(raw, plan, b, n):
    """Rules 1 - 4 on one frame raw [raw_h, raw_w, 3] from the plan's tables; returns [H, W, 3] uint8."""
    H, W = plan.final_dim
    k = np.arange(plan.col_taps.shape[2])

    def one_pass(img, first, count, taps):                 # along axis 1 of img [rows, in, 3]
        idx = np.clip(first[None] + k[:, None], 0, img.shape[1] - 1)
        t = np.where(k[:, None] < count[None], taps, 0).astype(np.int64)
        acc = (1 << 21) + np.einsum("ko,rkoc->roc", t, img[:, idx].astype(np.int64))
        return np.clip(acc >> 22, 0, 255).astype(np.uint8)

    hor = one_pass(raw, plan.col_first[b, n], plan.col_count[b, n], plan.col_taps[b, n])
    res = one_pass(hor.transpose(1, 0, 2), plan.row_first[b, n], plan.row_count[b, n], plan.row_taps[b, n])
    res = res.transpose(1, 0, 2)
    a0, a1, a2, a3, a4, a5, _x0, _y0, _nw, _nh, flip = (int(v) for v in plan.consts[b, n, :11])
    if flip:
        res = res[:, ::-1]
    y, x = np.mgrid[:H, :W]
    sx, sy = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    return np.where(inside[..., None], res[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], 0).astype(np.uint8)


def oracle_u8(raw, plan):
    return np.stack([np.stack([apply_plan(raw[b, n], plan, b, n) for n in range(plan.N)]) for b in range(plan.B)])


def normalise(u8, to_rgb, mean=MEAN, std=STD):
    """Rule 5 in numpy fp32: [B, N, H, W, 3] uint8 -> [B, N, 3, H, W]."""
    planes = []
    for c in range(3):
        src = u8[..., 2 - c if to_rgb else c].astype(f32)
        planes.append((src - f32(mean[c])) * f32(1.0 / np.float64(std[c])))
    out = np.stack(planes, 2)
    assert out.dtype == f32
    return out


def bf16_bits(x):
    """Round-to-nearest-even bf16 bit patterns of finite fp32 values, as int16."""
    u = np.ascontiguousarray(x).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def tup(raw_hw, resize, x0, y0, final, flip, rotate):
    H, W = final
    return (resize, (int(raw_hw[1] * resize), int(raw_hw[0] * resize)), (x0, y0, x0 + W, y0 + H), flip, rotate)


def fixture_case(name):
    g = np.load(GOLDEN)
    raw_h, raw_w, H, W = (int(v) for v in g[f"{name}_dims"])
    table = g[f"{name}_augs"]
    augs = [[(float(r[0]), (int(r[1]), int(r[2])), tuple(int(v) for v in r[3:7]), bool(r[7]), float(r[8]))
             for r in row] for row in table]
    return dict(raw_dim=(raw_h, raw_w), final_dim=(H, W), augs=augs, u8=g[f"{name}_u8"], ida=g[f"{name}_ida"],
                raw=raw_frames(len(augs), len(augs[0]), raw_h, raw_w))


# ----------------------------------------------------------------------------------------------------- CPU
@pytest.fixture(scope="module")
def lib():
    build_library(verbose=False)
    return _capi.load()


@pytest.mark.parametrize("name", CASES)
def test_plan_applier_reproduces_every_byte_of_the_reference_images(name):
    fx = fixture_case(name)
    plan = I.plan_camera_images(fx["augs"], fx["raw_dim"], fx["final_dim"])
    for k in I._TABLES:
        assert getattr(plan, k).dtype == np.int32, k
    B, N, (H, W) = plan.B, plan.N, plan.final_dim
    assert plan.col_taps.shape == (B, N, _capi.VAMP_IMG_MAX_TAPS, W) and plan.row_first.shape == (B, N, H)
    assert plan.device_tables is None                                  # pure host work
    got = oracle_u8(fx["raw"], plan)
    assert got.shape == fx["u8"].shape and np.array_equal(got, fx["u8"]), int((got != fx["u8"]).sum())
    assert fx["u8"].any()


def test_fixture_names_its_pillow_and_covers_the_issue_cases():
    g = np.load(GOLDEN)
    assert str(g["pillow_version"]) == "12.2.0"
    a, b, c = (fixture_case(n) for n in CASES)
    assert a["u8"].shape == (2, 3, 32, 88, 3) and b["u8"].shape == (1, 2, 16, 20, 3) and c["u8"].shape == (1, 2, 16, 24, 3)
    tuples = [t for fx in (a, b, c) for row in fx["augs"] for t in row]
    assert len({t for t in map(repr, a["augs"][0] + a["augs"][1])}) == 6
    assert {t[3] for t in tuples} == {True, False} and {-5.4, 0.0, 3.7} <= {t[4] for t in tuples}
    assert any(t[2][1] < 0 for t in tuples) and any(t[2][2] > t[1][0] for t in tuples)
    assert {t[0] for t in c["augs"][0]} == {1.3, 1.0} and (b["raw_dim"][1] * 3) % 2 == 1


@pytest.mark.parametrize("name", CASES)
def test_ida_mats_equal_the_reference_matrices(name):
    fx = fixture_case(name)
    got = I.ida_mats(fx["augs"])
    assert got.dtype == torch.float32 and tuple(got.shape) == fx["ida"].shape
    assert torch.equal(got.view(torch.int32), torch.from_numpy(fx["ida"]).view(torch.int32))


def _desc(**kw):
    d = _capi.VampImageDesc()
    d.B, d.N, d.raw_h, d.raw_w, d.H, d.W = 2, 3, 90, 160, 32, 88
    d.raw_row_stride, d.raw_n_stride, d.raw_b_stride = 480, 480 * 90, 480 * 90 * 3
    d.taps_x = d.taps_y = 16
    d.foot_w, d.foot_h, d.out_dtype, d.to_rgb = 180, 30, _capi.VAMP_F32, 1
    for c in range(3):
        d.mean[c], d.std_inv[c] = 100.0, 0.02
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_entry_points_reject_bad_arguments_without_gpu(lib):
    assert C.sizeof(_capi.VampImageDesc) == 104
    fake = [C.c_void_p(0x1000 * (i + 1)) for i in range(11)]          # never dereferenced: every check comes first
    call = lambda d, a, nbytes=1 << 40: lib.vamp_camera_images(C.byref(d), *a, nbytes, None)
    zero = _capi.VampImageDesc()
    assert lib.vamp_camera_images_workspace_bytes(C.byref(zero)) == 0
    assert lib.vamp_camera_images_workspace_bytes(None) == 0
    assert lib.vamp_camera_images(None, *fake, 1 << 40, None) == -1 and b"desc is NULL" in lib.vamp_last_error()
    assert call(zero, fake) == -1 and b"B must be in [1, 4096]" in lib.vamp_last_error()
    for field, value, message in (("N", 17, b"N must be in [1, 16]"), ("raw_w", 0, b"raw_h, raw_w must be"),
                                  ("W", 4097, b"H, W must be"), ("taps_x", 17, b"outside the library's range"),
                                  ("taps_y", 0, b"taps_x, taps_y"), ("foot_w", 273, b"outside the library's range"),
                                  ("foot_h", 49, b"foot_w, foot_h"), ("out_dtype", _capi.VAMP_F16, b"out_dtype"),
                                  ("to_rgb", 2, b"to_rgb"), ("raw_row_stride", 479, b"raw_row_stride"),
                                  ("raw_n_stride", -1, b"must not be negative")):
        bad = _desc(**{field: value})
        assert lib.vamp_camera_images_workspace_bytes(C.byref(bad)) == 0, field
        assert call(bad, fake) == -1 and message in lib.vamp_last_error(), (field, lib.vamp_last_error())
    nan = _desc()
    nan.std_inv[1] = float("inf")
    assert call(nan, fake) == -1 and b"finite" in lib.vamp_last_error()
    d = _desc()
    need = lib.vamp_camera_images_workspace_bytes(C.byref(d))
    assert need == 2 * 3 * 32 * 272                                    # align16(3 * 88) = 272 bytes per staging row
    assert call(d, fake[:8] + [None, None] + fake[10:]) == -1 and b"both NULL" in lib.vamp_last_error()
    assert call(d, fake[:8] + [None] + fake[9:]) == -1 and b"exactly when out_dtype" in lib.vamp_last_error()
    assert call(_desc(out_dtype=_capi.VAMP_IMG_OUT_NONE), fake) == -1 and b"exactly when" in lib.vamp_last_error()
    assert call(d, [None] + fake[1:]) == -1 and b"raw or a plan table is NULL" in lib.vamp_last_error()
    assert call(d, fake[:4] + [None] + fake[5:]) == -1 and b"plan table is NULL" in lib.vamp_last_error()
    assert call(d, fake[:8] + [C.c_void_p(0x9004)] + fake[9:]) == -1 and b"16-byte aligned" in lib.vamp_last_error()
    assert call(d, fake, need - 1) == -2 and b"workspace" in lib.vamp_last_error()
    assert call(d, fake[:10] + [None], need) == -2
    with pytest.raises(_capi.VampireHipError, match="vamp_camera_images failed with code -1"):
        _capi.checked().vamp_camera_images(zero, *([None] * 11), 0, None)


def test_plan_refuses_what_the_library_cannot_do():
    raw, final = (90, 160), (32, 88)
    ok = tup(raw, 0.5, 0, 3, final, False, 3.0)
    I.plan_camera_images([[ok]], raw, final)
    with pytest.raises(ValueError, match="rotate"):
        I.plan_camera_images([[tup(raw, 0.5, 0, 3, final, False, 60)]], raw, final)
    with pytest.raises(ValueError, match="rotate"):
        I.plan_camera_images([[tup(raw, 0.5, 0, 3, final, False, -45.0)]], raw, final)
    with pytest.raises(ValueError, match="outside its range"):
        I.plan_camera_images([[tup(raw, 0.2, 0, 0, final, False, 0)]], raw, final)
    with pytest.raises(ValueError, match="crop"):
        I.plan_camera_images([[(0.5, (80, 45), (0, 3, 80, 35), False, 0)]], raw, final)
    with pytest.raises(ValueError):
        I.plan_camera_images([[ok], [ok, ok]], raw, final)
    # a plan made at resize 0.55 has no room for 0.386 unless it was told; update keeps the shapes
    plan = I.plan_camera_images([[tup(raw, 0.55, 0, 3, final, False, 0)]], raw, final)
    small = [[tup(raw, 0.386, 0, 0, final, True, 0)]]
    with pytest.raises(ValueError, match="resize_min"):
        plan.update(small)
    roomy = I.plan_camera_images([[tup(raw, 0.55, 0, 3, final, False, 0)]], raw, final, resize_min=0.386)
    roomy.update(small)
    fresh = I.plan_camera_images(small, raw, final)
    assert roomy.foot_w >= fresh.foot_w and roomy.foot_h >= fresh.foot_h
    assert all(np.array_equal(getattr(roomy, k), getattr(fresh, k)) for k in I._TABLES)
    with pytest.raises(ValueError):
        roomy.update([[ok, ok]])


def test_python_interface_refuses_cpu_tensors_and_wrong_arguments():
    raw, final = (30, 40), (16, 24)
    plan = I.plan_camera_images([[tup(raw, 1.0, 8, 7, final, False, 0)]], raw, final)
    with pytest.raises(_capi.VampireHipError):
        I.camera_images(torch.zeros(1, 1, 30, 40, 3, dtype=torch.uint8), plan)


# ----------------------------------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu()


def assert_images(out, u8, want_u8, to_rgb, what=""):
    """out: fp32 or bf16 [B, N, 3, H, W]; u8: [B, N, H, W, 3] from the device; want_u8: numpy."""
    assert u8.dtype == torch.uint8 and torch.equal(u8.cpu(), torch.from_numpy(want_u8)), what
    want = normalise(want_u8, to_rgb)
    assert tuple(out.shape) == want.shape, what
    if out.dtype == torch.float32:
        assert torch.equal(bits(out), torch.from_numpy(want.view(np.int32))), what
    else:
        assert out.dtype == torch.bfloat16 and torch.equal(bits(out), torch.from_numpy(bf16_bits(want))), what


@gpu
@pytest.mark.parametrize("to_rgb", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_fixture_images(dev, name, to_rgb):
    fx = fixture_case(name)
    plan = I.plan_camera_images(fx["augs"], fx["raw_dim"], fx["final_dim"]).to(dev)
    raw = torch.from_numpy(fx["raw"]).to(dev)
    out, u8 = I.camera_images(raw, plan, to_rgb=to_rgb, out_u8=True)
    assert_images(out, u8, fx["u8"], to_rgb, name)
    half, u8b = I.camera_images(raw, plan, to_rgb=to_rgb, dtype=torch.bfloat16, out_u8=True)
    assert_images(half, u8b, fx["u8"], to_rgb, name)
    only = I.camera_images(raw, plan, to_rgb=to_rgb)
    assert torch.equal(bits(only), bits(out))
    none, u8c = I.camera_images(raw, plan, dtype=None, out_u8=True)
    assert none is None and torch.equal(u8c, u8)


RESIZES, ROTATES = (0.386, 0.44, 0.55, 1.0, 1.3), (-5.4, 0, 5.4)


def sweep_augs(raw_hw, final):
    """5 x 6 tuples: every (resize, rotate, flip); the crop alternates between a window inside the resized image
    (where it fits) and one that overruns it at the right and at the top."""
    H, W = final
    rows, i = [], 0
    for resize in RESIZES:
        row = []
        for rotate, flip in itertools.product(ROTATES, (False, True)):
            new_w, new_h = int(raw_hw[1] * resize), int(raw_hw[0] * resize)
            if i % 2 == 0:
                x0, y0 = max(0, (new_w - W) // 2), max(0, new_h - H)
            else:
                x0, y0 = new_w - W + 5, -3
            row.append(tup(raw_hw, resize, x0, y0, final, flip, rotate))
            i += 1
        rows.append(row)
    return rows


@gpu
@pytest.mark.parametrize("final", [(18, 70), (20, 44)])
@pytest.mark.parametrize("raw_hw", [(37, 53), (64, 96), (90, 160)])
def test_sweep_against_the_plan_applier(dev, raw_hw, final):
    """Final sizes that are no multiple of the 8 x 64 tile (three row tiles; two column tiles and the element stores
    at W = 70, one column tile and the 16-byte stores at W = 44)."""
    augs = sweep_augs(raw_hw, final)
    raw = raw_frames(5, 6, *raw_hw)
    plan = I.plan_camera_images(augs, raw_hw, final)
    want = oracle_u8(raw, plan)
    assert want.any()
    out, u8 = I.camera_images(torch.from_numpy(raw).to(dev), plan.to(dev), out_u8=True)
    assert_images(out, u8, want, True, (raw_hw, final))


@gpu
def test_layouts_give_the_same_values_or_raise(dev):
    fx = fixture_case("b")                                             # 37 x 53: 159-byte rows
    plan = I.plan_camera_images(fx["augs"], fx["raw_dim"], fx["final_dim"]).to(dev)
    raw = torch.from_numpy(fx["raw"]).to(dev)
    plain, plain_u8 = I.camera_images(raw, plan, out_u8=True)
    assert_images(plain, plain_u8, fx["u8"], True)
    B, N, h, w, _ = raw.shape
    big = torch.full((B, N + 1, h + 5, w + 7, 3), 0xEE, dtype=torch.uint8, device=dev)
    big[:, 1:, 2:2 + h, 3:3 + w] = raw
    inner = big[:, 1:, 2:2 + h, 3:3 + w]
    off = torch.zeros(raw.numel() + 1, dtype=torch.uint8, device=dev)
    off[1:] = raw.reshape(-1)
    views = dict(slice_of_a_wider_and_taller_buffer=inner, misaligned=off[1:].view(raw.shape))
    assert not inner.is_contiguous() and inner.stride(2) == (w + 7) * 3 and views["misaligned"].data_ptr() % 4 == 1
    for name, view in views.items():
        got, got_u8 = I.camera_images(view, plan, out_u8=True)
        assert torch.equal(got_u8, plain_u8) and torch.equal(bits(got), bits(plain)), name
    planar = raw.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)       # channel-first memory
    assert planar.shape == raw.shape and not planar.is_contiguous()
    with pytest.raises(ValueError, match="dense along its last two axes"):
        I.camera_images(planar, plan)
    with pytest.raises(TypeError):
        I.camera_images(raw.float(), plan)
    with pytest.raises(ValueError):
        I.camera_images(raw[:, :1], plan)
    # an expanded batch: same values, or a raised error
    one = I.plan_camera_images([fx["augs"][0], fx["augs"][0]], fx["raw_dim"], fx["final_dim"]).to(dev)
    try:
        got, got_u8 = I.camera_images(raw.expand(2, *raw.shape[1:]), one, out_u8=True)
    except (ValueError, TypeError, _capi.VampireHipError):
        return
    assert torch.equal(got_u8[0], plain_u8[0]) and torch.equal(got_u8[1], plain_u8[0])


@gpu
def test_dirty_workspace_and_out_reuse_are_bitwise_repeatable(dev):
    from vampire_amd import _tensors
    fx = fixture_case("a")
    raw = torch.from_numpy(fx["raw"]).to(dev)
    other = [row[::-1] for row in fx["augs"][::-1]]
    plan = I.plan_camera_images(fx["augs"], fx["raw_dim"], fx["final_dim"]).to(dev)
    out, u8 = I.camera_images(raw, plan, out_u8=True)
    assert_images(out, u8, fx["u8"], True)
    keys = [k for k in _tensors._scratch if isinstance(k, tuple) and k[0] == "camera_images"]
    assert keys
    fresh, fresh_u8 = I.camera_images(raw, I.plan_camera_images(other, fx["raw_dim"], fx["final_dim"]).to(dev), out_u8=True)
    fresh, fresh_u8 = fresh.clone(), fresh_u8.clone()
    assert not torch.equal(fresh_u8, u8)
    plan.update(other)
    for _ in range(2):
        for k in keys:
            _tensors._scratch[k].fill_(0xFF)
        out.view(torch.uint8).fill_(0xFF)
        u8.fill_(0xFF)
        ptrs = (out.data_ptr(), u8.data_ptr())
        got, got_u8 = I.camera_images(raw, plan, out=out, out_u8=u8)
        assert got is out and got_u8 is u8 and ptrs == (out.data_ptr(), u8.data_ptr())
        assert torch.equal(got_u8, fresh_u8) and torch.equal(bits(got), bits(fresh))
    with pytest.raises(ValueError):
        I.camera_images(raw, plan, dtype=torch.bfloat16, out=out)      # a buffer of another dtype
    with pytest.raises(ValueError):
        I.camera_images(raw, plan, out=out[:, :2])                      # and of another shape


@gpu
def test_no_sync_and_graph_replay_follows_plan_update(dev):
    fx = fixture_case("a")
    raw = torch.from_numpy(fx["raw"]).to(dev)
    other = [row[::-1] for row in fx["augs"][::-1]]
    plan = I.plan_camera_images(fx["augs"], fx["raw_dim"], fx["final_dim"]).to(dev)
    flat = plan._flat.data_ptr()
    out, u8 = I.camera_images(raw, plan, out_u8=True)                  # (the workspace exists from here on)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        I.camera_images(raw, plan, out=out, out_u8=u8)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            I.camera_images(raw, plan, out=out, out_u8=u8)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            I.camera_images(raw, plan, out=out, out_u8=u8)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_images(out, u8, fx["u8"], True)
    plan.update(other)
    assert plan._flat.data_ptr() == flat                               # the same device buffer, refilled
    out.zero_()
    u8.zero_()
    g.replay()
    torch.cuda.synchronize()
    eager, eager_u8 = I.camera_images(raw, I.plan_camera_images(other, fx["raw_dim"], fx["final_dim"]).to(dev), out_u8=True)
    assert torch.equal(u8, eager_u8) and torch.equal(bits(out), bits(eager))
    want = oracle_u8(fx["raw"], plan)
    assert not np.array_equal(want, fx["u8"])
    assert_images(out, u8, want, True)


@gpu
def test_fill_train_images_goes_with_fill_train_labels(dev):
    from vampire_amd import labels as L
    from vampire_amd import multitask as M
    cfg = CFG_TINY
    H, W = cfg.final_dim
    raw_hw = (90, 160)
    batch = M.synthetic_batch(cfg, 2, seed=3, device=dev, num_points=500)
    augs = [[tup(raw_hw, 0.55 - 0.02 * n, 0, 10 - n, (H, W), bool((b + n) % 2), (n - 2) * 1.8)
             for n in range(cfg.num_cams)] for b in range(2)]
    raw = torch.from_numpy(raw_frames(2, cfg.num_cams, *raw_hw)).to(dev)
    full = I.fill_train_images(batch, raw, augs, cfg)
    assert len(full) == len(batch)
    for i in range(len(batch)):
        if i == 0:
            assert full[0].shape == batch[0].shape and full[0].dtype == batch[0].dtype and full[0].device == batch[0].device
        elif i == 1:
            assert set(full[1]) == set(batch[1])
            for k in batch[1]:
                if k == "ida_mats":
                    assert full[1][k].shape == batch[1][k].shape and full[1][k].dtype == batch[1][k].dtype
                    assert full[1][k].device == batch[1][k].device
                else:
                    assert full[1][k] is batch[1][k], k
        else:
            assert full[i] is batch[i], i
    plan = I.plan_camera_images(augs, raw_hw, (H, W)).to(dev)
    direct = I.camera_images(raw, plan)
    assert torch.equal(bits(full[0][:, 0]), bits(direct))
    assert_images(direct, I.camera_images(raw, plan, dtype=None, out_u8=True)[1], oracle_u8(raw.cpu().numpy(), plan), True)
    assert torch.equal(full[1]["ida_mats"][:, 0].cpu(), I.ida_mats(augs))
    # the labels of the same augmentation values, on the batch that already carries the images
    both = L.fill_train_labels(full, cfg, augs, raw_dim=raw_hw)
    assert both[0] is full[0] and both[6].shape == batch[6].shape and both[6].shape[-2:] == both[0].shape[-2:]
