#!/usr/bin/env python3
"""Camera front end of a StereoRig on a KITTI-size batch (HIP events): us per pair for every pixel format x rectification x
resize, the bytes a pair must move and the rate that makes; then the rig end to end (device-resident BGR frames -> d1)
against the engine alone on the gray versions of the same frames, alternated in one process.

    python tools/rig_time.py [--batch 64] [--reps 20] [--out profiles/rig_time.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))  # test_legacy_entry imports pyoracle
PKG = "low-cost-hardware-accelerated-vision-based-depth-perception-for-real-time-applications_amd"
COPY_CEILING = 6.29e12  # B/s, float4 copy measured on MI355X (the copy ceiling of MI355X_MICROARCH.md)
CH = {"bgra": 4, "bgr": 3, "rgb": 3, "gray": 1}

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--e2e-reps", type=int, default=5)
ap.add_argument("--out", default="")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
from test_legacy_entry import _gray_cv4  # noqa: E402

W, H, B = 1242, 375, a.batch
g = os.path.join(ROOT, "tests", "golden")
rgb_l = np.asarray(Image.open(os.path.join(g, "kitti0_color_left.png")))
rgb_r = np.asarray(Image.open(os.path.join(g, "kitti0_color_right.png")))
rng = np.random.default_rng(0)
L = np.stack([np.roll(rgb_l, int(rng.integers(0, 50)), axis=1) for _ in range(B)])
R = np.stack([np.roll(rgb_r, int(rng.integers(0, 50)), axis=1) for _ in range(B)])


_sized = {}


def frames(fmt, x, src):
    if src != (W, H):
        key = (id(x), src)
        if key not in _sized:
            _sized[key] = np.stack([np.asarray(Image.fromarray(f).resize(src, Image.BILINEAR)) for f in x])
        x = _sized[key]
    if fmt == "bgr":
        x = x[..., ::-1]
    elif fmt == "bgra":
        x = np.concatenate([x[..., ::-1], np.full(x.shape[:3] + (1,), 255, np.uint8)], -1)
    elif fmt == "gray":
        x = _gray_cv4(x)
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def time_events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)  # us
    return float(np.median(ts)), float(np.min(ts))


res = {"batch": B, "width": W, "height": H, "copy_ceiling_Bps": COPY_CEILING, "frontend": [], "end_to_end": {}}
rigs = {rect: rigmod.StereoRig(W, H, rectify=rect) for rect in (False, True)}
for resize, src in (("none", (W, H)), ("2x", (2 * W, 2 * H)), ("1.5x", (W * 3 // 2, H * 3 // 2))):
    for fmt in ("bgra", "bgr", "rgb", "gray"):
        l, r = frames(fmt, L, src), frames(fmt, R, src)
        for rect in (False, True):
            rig = rigs[rect]
            med, best = time_events(lambda: rig.frontend(l, r, pixel_format=fmt), a.reps)
            sw, sh = src
            # bytes a pair must move: both source frames read once, both gray images written; the remap adds both maps' 8 B per pixel
            need = 2 * sw * sh * CH[fmt] + 2 * W * H + (2 * 8 * W * H if rect else 0)
            row = {"format": fmt, "rectify": rect, "resize": resize, "src": [sw, sh], "us_per_pair": med / B, "us_per_pair_best": best / B,
                   "bytes_per_pair": need, "GBps": need * B / (med * 1e-6) / 1e9}
            row["copy_ceiling_fraction"] = row["GBps"] * 1e9 / COPY_CEILING
            res["frontend"].append(row)
            print("%-5s rectify=%d resize=%-4s  %.3f us/pair (best %.3f)  %.1f MB/pair  %.0f GB/s  %.2f of the copy ceiling"
                  % (fmt, rect, resize, row["us_per_pair"], row["us_per_pair_best"], need / 1e6, row["GBps"], row["copy_ceiling_fraction"]), flush=True)
        del l, r
        torch.cuda.empty_cache()
for rig in rigs.values():
    rig.close()

# end to end: the rig (front end + engine) on BGR frames vs the engine alone on gray frames, alternated
lb, rb = frames("bgr", L, (W, H)), frames("bgr", R, (W, H))
lg, rg = frames("gray", L, (W, H)), frames("gray", R, (W, H))
rig = rigmod.StereoRig(W, H)
engine = eng.StereoEngine(W, H, eng.SvParams.driver(255))
d1 = torch.zeros((B, H, W), dtype=torch.float32, device="cuda")
rig.disparity(lb, rb, pixel_format="bgr")
engine.process_device(lg, rg, d1=d1, want_d2=False)
t_rig, t_eng = [], []
for _ in range(a.e2e_reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rig.disparity(lb, rb, pixel_format="bgr")
    torch.cuda.synchronize()
    t_rig.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    engine.process_device(lg, rg, d1=d1, want_d2=False)
    torch.cuda.synchronize()
    t_eng.append(time.perf_counter() - t0)
e2e = {"rig_pairs_per_s": B / float(np.median(t_rig)), "engine_pairs_per_s": B / float(np.median(t_eng))}
e2e["ratio"] = e2e["rig_pairs_per_s"] / e2e["engine_pairs_per_s"]
res["end_to_end"] = e2e
print("end to end, batch %d: rig (BGR -> d1) %.0f pairs/s, engine alone (gray -> d1) %.0f pairs/s, ratio %.3f"
      % (B, e2e["rig_pairs_per_s"], e2e["engine_pairs_per_s"], e2e["ratio"]))
engine.close()
rig.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
