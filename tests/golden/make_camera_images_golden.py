#!/usr/bin/env python3
"""Golden images for the camera image transform (tests/test_camera_images.py), made by the reference loader's own
`img_transform` IN THIS CONTAINER with the Pillow that is installed here (its version is stored in the file: the
reference does not pin one).  The reference module cannot be imported (nuscenes-devkit, mmcv and mmdet3d are absent),
so /root/reference/src/datasets/nusc_det_seg_dataset.py is parsed with `ast` at run time and only the definitions of
`get_rot` and `img_transform` are executed, with `Image`, `np` and `torch`; this script holds none of their text.
mmcv.imnormalize is absent too: the normalisation is not part of the fixture.  Run once here; the .npz travels, the
reference does not.

The raw frames come from `raw_frames`, an integer formula of (b, n, y, x, c) that tests/test_camera_images.py writes
out too, so the file holds no input image.

The script asserts the conditions the tests rely on, measured with a numpy applier of the plan tables of
vampire_amd.images.plan_camera_images (rules 1 - 4 of include/vampire_hip.h), which must reproduce every byte of
Pillow's images: over all cases, both passes of the resize clip at 0 and at 255; a tap window is cut at each of the
four image borders; one case has y0 < 0 and one x0 + W > newW; in every rotated case some but fewer than 10 % of the
pixels are rotation fill."""
import ast
import os
import sys

import numpy as np
import PIL
import torch
from PIL import Image

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vampire_amd.images import plan_camera_images  # noqa: E402

REF = "/root/reference/src/datasets/nusc_det_seg_dataset.py"
WANT = ("get_rot", "img_transform")
tree = ast.parse(open(REF).read())
defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in WANT]
assert sorted(n.name for n in defs) == sorted(WANT)
ref = {"np": np, "torch": torch, "Image": Image}
exec(compile(ast.Module(body=defs, type_ignores=[]), REF, "exec"), ref)


def raw_frames(B, N, h, w):
    """[B, N, h, w, 3] uint8: saturated blocks (hard edges, so that the bicubic overshoots below 0 and above 255)
    with hashed texture in every third 16 x 8 region."""
    b, n, y, x, c = np.ogrid[:B, :N, :h, :w, :3]
    b, n, y, x, c = (v.astype(np.int64) for v in (b, n, y, x, c))
    block = ((x // 5 + y // 3 + n + b) % 2) * 255 + 0 * c
    tex = ((x * 7 + y * 13 + c * 31 + n * 5 + b * 3 + 1) * 2654435761 % 4294967296) >> 24
    return np.where((x // 16 + y // 8 + n) % 3 == 0, tex, block).astype(np.uint8)


def apply_plan(raw, plan, b, n, stats=None):
    """Rules 1 - 4 on one frame raw [raw_h, raw_w, 3] from the plan's tables; returns [H, W, 3] uint8."""
    H, W = plan.final_dim
    k = np.arange(plan.col_taps.shape[2])

    def one_pass(img, first, count, taps, name):          # along axis 1 of img [rows, in, 3]
        idx = np.clip(first[None] + k[:, None], 0, img.shape[1] - 1)               # [K, out]
        t = np.where(k[:, None] < count[None], taps, 0).astype(np.int64)
        acc = (1 << 21) + np.einsum("ko,rkoc->roc", t, img[:, idx].astype(np.int64))
        v = acc >> 22
        if stats is not None:
            stats[name + "_lo"] = stats.get(name + "_lo", 0) + int((v < 0).sum())
            stats[name + "_hi"] = stats.get(name + "_hi", 0) + int((v > 255).sum())
        return np.clip(v, 0, 255).astype(np.uint8)

    hor = one_pass(raw, plan.col_first[b, n], plan.col_count[b, n], plan.col_taps[b, n], "h")     # [raw_h, W, 3]
    res = one_pass(hor.transpose(1, 0, 2), plan.row_first[b, n], plan.row_count[b, n], plan.row_taps[b, n], "v")
    res = res.transpose(1, 0, 2)                                                                   # [H, W, 3]
    a0, a1, a2, a3, a4, a5, _x0, _y0, _nw, _nh, flip = (int(v) for v in plan.consts[b, n, :11])
    if flip:
        res = res[:, ::-1]
    y, x = np.mgrid[:H, :W]
    sx, sy = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    if stats is not None:
        stats["fill"] = float(1.0 - inside.mean())
    return np.where(inside[..., None], res[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], 0).astype(np.uint8)


def tup(raw_hw, resize, x0, y0, final, flip, rotate):
    H, W = final
    return (resize, (int(raw_hw[1] * resize), int(raw_hw[0] * resize)), (x0, y0, x0 + W, y0 + H), flip, rotate)


CASES = {
    # name: (raw (h, w), final (H, W), augs[b][n])
    "a": ((90, 160), (32, 88), lambda r, f: [
        [tup(r, 0.55, 0, 17, f, False, 0), tup(r, 0.386, 0, 2, f, True, -5.4), tup(r, 0.44, 0, 7, f, False, 3.7)],
        [tup(r, 0.5, 0, -3, f, True, 3.7), tup(r, 0.55, 0, 10, f, True, 0), tup(r, 0.47, 0, 10, f, False, -5.4)]]),
    "b": ((37, 53), (16, 20), lambda r, f: [
        [tup(r, 0.45, 5, -2, f, False, 5.4), tup(r, 0.6, 11, 6, f, True, -5.4)]]),
    "c": ((30, 40), (16, 24), lambda r, f: [
        [tup(r, 1.3, 14, 11, f, False, 0), tup(r, 1.0, 8, 7, f, True, 4.5)]]),
}

out = {"pillow_version": np.array(PIL.__version__)}
total, cut, neg_y0, over_x = {}, set(), False, False
for name, (raw_hw, final, make) in CASES.items():
    augs = make(raw_hw, final)
    B, N = len(augs), len(augs[0])
    raw = raw_frames(B, N, *raw_hw)
    plan = plan_camera_images(augs, raw_hw, final)
    H, W = final
    imgs, mats = np.zeros((B, N, H, W, 3), np.uint8), np.zeros((B, N, 4, 4), np.float32)
    table = np.zeros((B, N, 9))
    for b in range(B):
        for n in range(N):
            resize, dims, crop, flip, rotate = augs[b][n]
            img, mat = ref["img_transform"](Image.fromarray(raw[b, n]), resize, dims, crop, flip, rotate)
            imgs[b, n], mats[b, n] = np.array(img), mat.numpy()
            table[b, n] = (resize, dims[0], dims[1], *crop, float(flip), rotate)
            stats = {}
            mine = apply_plan(raw[b, n], plan, b, n, stats)
            assert np.array_equal(mine, imgs[b, n]), (name, b, n, int((mine != imgs[b, n]).sum()))
            for key in ("h_lo", "h_hi", "v_lo", "v_hi"):
                total[key] = total.get(key, 0) + stats[key]
            if rotate:
                assert 0.0 < stats["fill"] < 0.10, (name, b, n, stats["fill"])
            # a tap window cut at a border: fewer taps than the window of an interior output of the same axis
            cc, rc = plan.col_count[b, n], plan.row_count[b, n]
            cf, rf = plan.col_first[b, n], plan.row_first[b, n]
            if ((cc > 0) & (cf == 0) & (cc < cc.max())).any():
                cut.add("left")
            if ((cc > 0) & (cf + cc == raw_hw[1]) & (cc < cc.max())).any():
                cut.add("right")
            if ((rc > 0) & (rf == 0) & (rc < rc.max())).any():
                cut.add("top")
            if ((rc > 0) & (rf + rc == raw_hw[0]) & (rc < rc.max())).any():
                cut.add("bottom")
            neg_y0 |= crop[1] < 0
            over_x |= crop[2] > dims[0]
    out.update({f"{name}_u8": imgs, f"{name}_ida": mats, f"{name}_augs": table,
                f"{name}_dims": np.array([*raw_hw, *final], np.int32)})
    print(f"{name}: {B} x {N} frames {raw_hw} -> {final}, all bytes equal to the plan applier's")

print("clipped outputs:", total, "cut windows:", sorted(cut))
assert all(total[k] > 0 for k in ("h_lo", "h_hi", "v_lo", "v_hi")), total
assert cut == {"left", "right", "top", "bottom"}, cut
assert neg_y0 and over_x

path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "camera_images.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
