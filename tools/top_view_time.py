#!/usr/bin/env python3
"""Bird's-eye views on KITTI maps (HIP events, median of --reps samples, each sample --inner calls back to back): for B = 1, 16, 256
and both modes, on the CLI's grid (disparity "d1", camera-to-vehicle rotation, x 0..40, y -20..20, z -1.4..1.0, scale 10):
  (a) us per pair of the fused disparity -> grid call (memset, rasteriser, finalize), with and without the wave combine;
  (b) us per pair of the unfused path: reproject to an f64 cloud, then the points entry (each timed on its own, summed);
  (c) grid atomics issued per pair with and without the combine (sv_debug_top_view's counter);
  (d) rig.top_view against rig.disparity, pairs/s at B = 64 on device-resident BGR frames, alternated.
The maps are the engine's d1 of the committed KITTI frames (tests/golden), repeated to fill the batch.

    python tools/top_view_time.py [--reps 20] [--inner 5] [--out profiles/top_view_time.json]
"""
import argparse
import ctypes
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
PKG = "low-cost-hardware-accelerated-vision-based-depth-perception-for-real-time-applications_amd"

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--e2e-reps", type=int, default=5)
ap.add_argument("--batches", default="1,16,256")
ap.add_argument("--out", default="")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
sv = importlib.import_module(PKG + ".stereo_vision.sv")
L = eng.top_view_lib()
W, H = 1242, 375
G = os.path.join(ROOT, "tests", "golden")


def png(name):
    return np.asarray(Image.open(os.path.join(G, name)))


def gray3(name):
    g = png(name)
    return np.ascontiguousarray(np.repeat(g[..., None], 3, -1))


ls = [png("kitti0_color_left.png")] + [gray3("kitti%d_left.png" % k) for k in (1, 2, 3, 4)]
rs = [png("kitti0_color_right.png")] + [gray3("kitti%d_right.png" % k) for k in (1, 2, 3, 4)]
rig = rigmod.StereoRig(W, H)
d1_all = rig.disparity(torch.from_numpy(np.stack(ls)).cuda(), torch.from_numpy(np.stack(rs)).cuda(), pixel_format="rgb")
Q = rig.Q.copy()
q = np.ascontiguousarray(Q, np.float64).reshape(16)
XR = np.ascontiguousarray(sv.CAMERA_TO_VEHICLE, np.float64).reshape(9)
GRID = sv.CLI_TOP_VIEW


def time_events(fn, reps, inner):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / inner)  # us per call
    return float(np.median(ts)), float(np.min(ts))


res = {"width": W, "height": H, "grid": {k: list(v) if isinstance(v, tuple) else v for k, v in GRID.items()}, "disparity": "d1",
       "reps": a.reps, "inner": a.inner, "rows": [], "rig": {}}
for B in [int(b) for b in a.batches.split(",")]:
    d1 = d1_all[torch.arange(B) % d1_all.shape[0]].contiguous()
    for mode in ("reference", "count"):
        spec, rows, cols = eng.top_view_spec(mode=mode, disparity="d1", **GRID)
        out = torch.empty((B, rows, cols), dtype=torch.uint8 if mode == "reference" else torch.int32, device="cuda")
        nbytes = L.sv_top_view_workspace_bytes(ctypes.byref(spec), B)
        ws = torch.empty((max(nbytes, 8) // 8,), dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def fused():
            rc = L.sv_top_view_disparity_device(d1.data_ptr(), B, W, H, q.ctypes.data, XR.ctypes.data, None, ctypes.byref(spec), out.data_ptr(),
                                                ws.data_ptr(), nbytes, st)
            assert rc == 0

        row = {"batch": B, "mode": mode, "workspace_bytes_per_pair": nbytes // B}
        counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        for combine in (1, 0):
            L.sv_debug_top_view(combine, None)
            med, best = time_events(fused, a.reps, a.inner)
            row["fused_us_per_pair" + ("" if combine else "_no_combine")] = med / B
            row["fused_us_per_pair_best" + ("" if combine else "_no_combine")] = best / B
            counter.zero_()
            torch.cuda.synchronize()
            L.sv_debug_top_view(combine, ctypes.c_void_p(counter.data_ptr()))
            fused()
            torch.cuda.synchronize()
            row["atomics_per_pair" + ("" if combine else "_no_combine")] = int(counter.item()) / B
        L.sv_debug_top_view(1, None)
        ref_grid = out.clone()
        # unfused: reproject (null stream, waits) to an f64 cloud, then the points entry on it
        pts = torch.empty((B, H, W, 3), dtype=torch.float64, device="cuda")
        Lr = eng.lib()

        def reproject():
            assert Lr.sv_reproject_batch_device(d1.data_ptr(), B, W, H, q.ctypes.data, XR.ctypes.data, None, None, pts.data_ptr()) == 0

        def points():
            assert L.sv_top_view_points_device(pts.data_ptr(), B, H * W, ctypes.byref(spec), out.data_ptr(), ws.data_ptr(), nbytes, st) == 0

        Lr.sv_reproject_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        # d1 mode of the fused call == the points entry on the cloud of d1 itself only where every d1 > 0; the timing is what matters
        # here, the equality of the dmap forms is tests/test_top_view.py's
        t_rep, _ = time_events(reproject, a.reps, a.inner)
        t_pts, _ = time_events(points, a.reps, a.inner)
        row["unfused_reproject_us_per_pair"] = t_rep / B
        row["unfused_points_us_per_pair"] = t_pts / B
        row["unfused_us_per_pair"] = (t_rep + t_pts) / B
        row["occupied_cells_pair0"] = int((ref_grid[0] > 0).sum().item())
        res["rows"].append(row)
        print("B=%-3d %-9s fused %.3f us/pair (no combine %.3f)  unfused %.3f (reproject %.3f + points %.3f)  atomics/pair %.0f (no combine %.0f)"
              % (B, mode, row["fused_us_per_pair"], row["fused_us_per_pair_no_combine"], row["unfused_us_per_pair"], row["unfused_reproject_us_per_pair"],
                 row["unfused_points_us_per_pair"], row["atomics_per_pair"], row["atomics_per_pair_no_combine"]), flush=True)
        del pts, ws, out
        torch.cuda.empty_cache()

# (d) rig.top_view vs rig.disparity, B = 64, device-resident BGR frames, alternated
B = 64
lb = torch.from_numpy(np.ascontiguousarray(np.stack([ls[k % 5] for k in range(B)])[..., ::-1])).cuda()
rb = torch.from_numpy(np.ascontiguousarray(np.stack([rs[k % 5] for k in range(B)])[..., ::-1])).cuda()
kw = dict(pixel_format="bgr", disparity="d1", transform=(sv.CAMERA_TO_VEHICLE, None), **GRID)
rig.disparity(lb, rb, pixel_format="bgr")
rig.top_view(lb, rb, **kw)
t_d, t_t = [], []
for _ in range(a.e2e_reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rig.disparity(lb, rb, pixel_format="bgr")
    torch.cuda.synchronize()
    t_d.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    rig.top_view(lb, rb, **kw)
    torch.cuda.synchronize()
    t_t.append(time.perf_counter() - t0)
e2e = {"batch": B, "disparity_pairs_per_s": B / float(np.median(t_d)), "top_view_pairs_per_s": B / float(np.median(t_t))}
e2e["ratio"] = e2e["top_view_pairs_per_s"] / e2e["disparity_pairs_per_s"]
res["rig"] = e2e
print("rig, batch %d: top_view %.0f pairs/s, disparity %.0f pairs/s, ratio %.3f" % (B, e2e["top_view_pairs_per_s"], e2e["disparity_pairs_per_s"], e2e["ratio"]))
rig.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
