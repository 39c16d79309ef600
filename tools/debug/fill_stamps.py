#!/usr/bin/env python3
"""Dev aid (GPU box, library built with -DVAMP_LIFT_STAMPS (tools/ablate.sh lift_bwd_cell.hip stamps=-DVAMP_LIFT_STAMPS)):
per-wave phase times of the lift backward's fill at cfg-B -- the mask wait, the row (with the first camera batch's
loads issued under it), the cells' arrival + issue of the atomics, the atomics' return, staging + stores."""
import os, sys, ctypes as C
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from vampire_amd.config import PRESETS
from vampire_amd import synthetic
from vampire_amd.ops import HotPath
from vampire_amd.geometry import lift_matrices
cfg = PRESETS["B"]; dev = torch.device("cuda:0"); hp = HotPath(cfg, dev)
s2e, K, ida = synthetic.camera_rig(cfg, 1)
lm = lift_matrices(s2e, K, ida, synthetic.bda_matrix(1)).to(dev)
depth, feat = synthetic.lift_inputs(cfg, 1, device=dev)
depth.requires_grad_(True); feat.requires_grad_(True)
go = torch.randn(1, cfg.mid_channels, cfg.vZ, cfg.vY, cfg.vX, device=dev)
for _ in range(3):
    depth.grad = None; feat.grad = None
    hp.lift(depth, feat, lm).backward(go)
torch.cuda.synchronize()
n = min(16384, (cfg.vZ * cfg.vY * cfg.vX + 63) // 64)
buf = np.zeros((n, 8), dtype=np.int64)
lib = hp.lib
lib.vamp_debug_read_fill_stamps.argtypes = [C.c_void_p, C.c_int]
assert lib.vamp_debug_read_fill_stamps(buf.ctypes.data, n) == 0
buf = buf[buf[:, 7] == 1]                       # the waves that had a camera
print("waves with a camera: %d of %d; lanes with a pair per wave: mean %.1f" % (len(buf), n, buf[:, 6].mean()))
names = ("mask wait", "row (+ camera loads issued)", "cells arrive, atomics issued", "atomics + cell starts return", "staging + stores")
tot = (buf[:, 5] - buf[:, 0]).astype(float)
print("wave life (s_memtime ticks): mean %.0f p50 %.0f p90 %.0f" % (tot.mean(), *np.percentile(tot, [50, 90])))
for i, nm in enumerate(names):
    v = (buf[:, i + 1] - buf[:, i]).astype(float)
    print("  %-30s mean %7.0f  p50 %7.0f  p90 %7.0f  share %.2f" % (nm, v.mean(), *np.percentile(v, [50, 90]), v.sum() / tot.sum()))
