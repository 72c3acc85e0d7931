#!/usr/bin/env python3
"""A voxel map carved by the sight lines of frames on a KITTI drive (HIP events, median of --reps samples, each sample --inner calls back
to back; min / max beside the median).  The maps are tools/voxel_map_time.py's: B = 256 frames from the rig (the engine's d1 of the
committed KITTI frames, cycled) along a gently turning trajectory, the CLI crop in vehicle axes, the frames' voxel rows with weights
inserted at voxel sizes 0.1 / 0.2 / 0.5 m.  Per size and reach (10 m and 20 m), sv_voxel_carve_device with the last --frames frames of
the drive under their own sequence numbers - the call that follows their insert -, margin 1, min_miss 2, ratio 0:
  (a) us per frame of the whole call on a pre-allocated miss tensor with apply = 0 and with apply = 1 (the second call of either finds
      the same work: an emptied voxel reads as last seen at 0, is counted against again and emptied again);
  (b) the kernels by difference: the call with batch = 0 is the zero and the apply kernel; the same on the map with its overflow flag
      set - the flag is put back afterwards - is the zero kernel and two launches that return at once; what the whole call takes beyond
      the call with batch = 0 is the ray kernel;
  (c) rays and steps per frame, the table look-ups (= steps) per microsecond of the ray kernel, and the miss atomics per frame, counted
      by one call with every weight 1; and the same call with the frames numbered from 0 - the same rays and look-ups, but hardly a
      voxel within reach is older than the frames, so next to no atomic is issued: what the look-ups cost alone;
  (d) the unfused form on the same device with torch ops: the map's sorted keys and last_seq from voxel_map_rows, per frame the
      transform, the cells and the rays, and per step k the cells, the keys, torch.searchsorted and an index_add - one Python loop over
      the steps.  Before anything is timed both forms must agree on the touched voxels and their miss.
It reports the times; it is not a gate, and a case in which the fused call is not faster is reported as such.

    timeout -k 10 900 python tools/voxel_carve_time.py [--reps 7] [--inner 2] [--out profiles/voxel_carve_time.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "low-cost-hardware-accelerated-vision-based-depth-perception-for-real-time-applications_amd"

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=2)
ap.add_argument("--batch", type=int, default=256, help="frames of the drive")
ap.add_argument("--frames", type=int, default=5, help="frames carved with per call: the last of the drive")
ap.add_argument("--sizes", default="0.1,0.2,0.5")
ap.add_argument("--reaches", default="10,20", help="metres")
ap.add_argument("--out", default="")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
svmod = importlib.import_module(PKG + ".stereo_vision.sv")
L, C = eng.voxel_map_lib(), eng.voxel_carve_lib()
W, H = 1242, 375
G = os.path.join(ROOT, "tests", "golden")
XR = np.ascontiguousarray(svmod.CAMERA_TO_VEHICLE)
LO, HI = svmod.CLI_CLOUD_CROP
ROWS = {0.05: 131072, 0.1: 65536, 0.2: 32768, 0.5: 8192}  # voxel size -> rows per frame of the voxel feed
MARGIN, MIN_MISS, RATIO = 1, 2, 0
ORIGIN = np.zeros(3)  # the camera's centre in vehicle axes: CAMERA_TO_VEHICLE only turns


def png(name):
    return np.asarray(Image.open(os.path.join(G, name)))


def gray3(name):
    return np.ascontiguousarray(np.repeat(png(name)[..., None], 3, -1))


ls = [png("kitti0_color_left.png")] + [gray3("kitti%d_left.png" % k) for k in (1, 2, 3, 4)]
rs = [png("kitti0_color_right.png")] + [gray3("kitti%d_right.png" % k) for k in (1, 2, 3, 4)]
rig = rigmod.StereoRig(W, H)
tl, tr = torch.from_numpy(np.stack(ls)).cuda(), torch.from_numpy(np.stack(rs)).cuda()
d1_all = rig.disparity(tl, tr, pixel_format="rgb")
Q = rig.Q.copy()
rig.close()
B, F = a.batch, a.frames
assert 1 <= F < B
sel = torch.arange(B) % d1_all.shape[0]
d1 = d1_all[sel].contiguous()
frame_no = np.arange(B, dtype=np.float64)
xyyaw = np.stack([0.8 * frame_no, 0.05 * frame_no, 0.002 * frame_no], -1)  # 204 m, turning by half a radian
poses_np = svmod.voxel_map_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2])
poses = torch.from_numpy(poses_np).cuda()
box_lo, box_hi = svmod.cli_voxel_map_box(xyyaw)
st = torch.cuda.current_stream().cuda_stream


def time_events(fn, reps, inner, per=1):
    for _ in range(2):
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
        ts.append(e0.elapsed_time(e1) * 1e3 / inner / per)
    return {"us": float(np.median(ts)), "min_max": [float(np.min(ts)), float(np.max(ts))]}


res = {"width": W, "height": H, "batch": B, "frames_per_call": F, "dtype": "f32", "margin": MARGIN, "min_miss": MIN_MISS, "ratio": RATIO, "box": [list(box_lo), list(box_hi)],
       "reps": a.reps, "inner": a.inner, "entry_bytes": 88, "voxel_match_lookups_per_us": [27000, 30000], "sizes": []}
for size in [float(s) for s in a.sizes.split(",")]:
    vox = eng.voxel_cloud_from_disparity(d1, Q, size, LO, HI, XR=XR, capacity=ROWS[size])
    assert (vox[5] >= 0).all().item(), "a frame holds more voxels than %d rows at size %g" % (ROWS[size], size)
    probe = svmod.voxel_map_params(box_lo, box_hi, size, 2 ** 24)
    buf = eng.voxel_map_new(probe)
    eng.voxel_map_insert(buf, probe, vox[0], None, vox[3], vox[5], poses)
    V = eng.voxel_map_stats(buf)[0]
    del buf
    torch.cuda.empty_cache()
    capacity = min(max(V + V // 8, 65536), 2 ** 26)  # voxel_map_time.py's rule
    params = svmod.voxel_map_params(box_lo, box_hi, size, capacity)
    spec, nbytes = eng.voxel_map_spec(params), L.sv_voxel_map_bytes(capacity)
    buf = eng.voxel_map_new(params)
    eng.voxel_map_insert(buf, params, vox[0], None, vox[3], vox[5], poses)
    fx, fn, fc, fp = vox[0][B - F:].contiguous(), vox[3][B - F:].contiguous(), vox[5][B - F:].contiguous(), poses[B - F:].contiguous()
    del vox
    torch.cuda.empty_cache()
    slots = int(L.sv_voxel_map_slots(capacity))
    miss = eng.voxel_carve_miss(buf, params)
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")
    rows = eng.voxel_map_rows(buf, params)
    vkeys, vlast = rows["key"], rows["last_seq"].long()  # ascending in key
    del rows
    lo_t, hi_t = torch.tensor(params["lo"], dtype=torch.float64, device="cuda"), torch.tensor(params["hi"], dtype=torch.float64, device="cuda")
    cells_t = torch.tensor(params["cells"], device="cuda")
    size_t = torch.tensor(size, dtype=torch.float64, device="cuda")  # a tensor: torch divides by a Python number as a product with its reciprocal
    entry = {"size": size, "voxels_in_the_map": V, "capacity": capacity, "table_slots": slots, "map_bytes": nbytes, "rows_per_frame": float(fc.sum().item()) / F, "reaches": []}

    def call(reach, apply=0, batch=F, weights=True, seq0=B - F):
        rc = C.sv_voxel_carve_device(buf.data_ptr(), nbytes, ctypes.byref(spec), fx.data_ptr(), 0, fn.data_ptr() if weights else None, fc.data_ptr(), fp.data_ptr(),
                                     ORIGIN.ctypes.data, batch, ROWS[size], seq0, reach, MARGIN, MIN_MISS, RATIO, apply, miss.data_ptr(), stats.data_ptr(), st)
        assert rc == 0, L.sv_last_error(None)

    def unfused(reach):
        """miss per row of voxel_map_rows with torch device ops: a frame at a time, a step at a time."""
        out = torch.zeros(len(vkeys), dtype=torch.int64, device="cuda")
        for b in range(F):
            k = int(fc[b].item())
            P, w, R = fx[b, :k].double(), fn[b, :k].long(), fp[b]
            O = torch.stack([((R[3 * j] * ORIGIN[0] + R[3 * j + 1] * ORIGIN[1]) + R[3 * j + 2] * ORIGIN[2]) + R[9 + j] for j in range(3)])
            if not (torch.isfinite(R).all() & ((O > lo_t) & (O < hi_t)).all()).item():
                continue
            c0 = torch.minimum(((O - lo_t) / size_t).long(), cells_t - 1)
            Pw = torch.stack([((R[3 * j] * P[:, 0] + R[3 * j + 1] * P[:, 1]) + R[3 * j + 2] * P[:, 2]) + R[9 + j] for j in range(3)], -1)
            keep = ((Pw > lo_t) & (Pw < hi_t)).all(-1) & (w > 0)
            d = torch.minimum(((Pw[keep] - lo_t) / size_t).long(), cells_t - 1) - c0
            nst = d.abs().max(1).values
            ray = nst <= reach
            d, nst, w = d[ray], nst[ray], w[keep][ray]
            ns = (nst - 1 - MARGIN).clamp(min=0)
            for step in range(1, int(ns.max().item()) + 1 if len(ns) else 1):
                on = ns >= step
                den = 2 * nst[on][:, None]
                c = c0 + torch.div(2 * step * d[on] + nst[on][:, None], den, rounding_mode="floor")
                key = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
                at = torch.searchsorted(vkeys, key).clamp(max=len(vkeys) - 1)
                hit = (vkeys[at] == key) & (vlast[at] < B - F + b)
                out.index_add_(0, at[hit], w[on][hit])
        return out

    for reach_m in [float(r) for r in a.reaches.split(",")]:
        reach = int(np.ceil(reach_m / size))
        assert reach <= svmod.VOXEL_CARVE_REACH_MAX
        # the two forms agree on the touched voxels and their miss
        call(reach)
        key, got = eng.voxel_carve_touched(buf, params, miss)
        counts = stats.cpu().tolist()
        slow = unfused(reach)
        assert torch.equal(key, vkeys[slow > 0]) and torch.equal(got, slow[slow > 0]), "the fused and the unfused form disagree at %g m, reach %g m: %d and %d touched, miss %d and %d" % (
            size, reach_m, len(key), int((slow > 0).sum().item()), int(got.sum().item()), int(slow.sum().item()))
        call(reach, weights=False)
        torch.cuda.synchronize()
        atomics = int(miss.sum().item())
        r = {"reach_m": reach_m, "reach_cells": reach, "rays_per_frame": counts[0] / F, "steps_per_frame": counts[1] / F, "touched": counts[2], "carved": counts[3],
             "miss_atomics_per_frame": atomics / F,
             "call_us_per_frame": time_events(lambda: call(reach), a.reps, a.inner, F),
             "zero_and_apply_us": time_events(lambda: call(reach, batch=0), a.reps, a.inner)}
        buf.view(torch.int32)[1] = 1  # the overflow flag: the ray and the apply kernel return at once
        r["zero_us"] = time_events(lambda: call(reach, batch=0), a.reps, a.inner)
        buf.view(torch.int32)[1] = 0
        r["apply_kernel_us"] = r["zero_and_apply_us"]["us"] - r["zero_us"]["us"]
        r["ray_kernel_us_per_frame"] = r["call_us_per_frame"]["us"] - r["zero_and_apply_us"]["us"] / F
        r["lookups_per_us"] = r["steps_per_frame"] / r["ray_kernel_us_per_frame"]
        # the same rays numbered from 0: the same look-ups, and no voxel within reach is older than the frames, so next to no atomic
        r["call_numbered_from_0_us_per_frame"] = time_events(lambda: call(reach, seq0=0), a.reps, a.inner, F)
        torch.cuda.synchronize()
        r["touched_numbered_from_0"] = int(stats[2].item())
        r["ray_kernel_without_atomics_us_per_frame"] = r["call_numbered_from_0_us_per_frame"]["us"] - r["zero_and_apply_us"]["us"] / F
        r["lookups_per_us_without_atomics"] = r["steps_per_frame"] / r["ray_kernel_without_atomics_us_per_frame"]
        r["unfused_us_per_frame"] = time_events(lambda: unfused(reach), max(a.reps // 2, 3), 1, F)
        r["unfused_over_fused"] = r["unfused_us_per_frame"]["us"] / r["call_us_per_frame"]["us"]
        r["fused_is_faster"] = bool(r["unfused_over_fused"] > 1)
        entry["reaches"].append(r)
    for r in entry["reaches"]:  # apply = 1 changes the map: behind everything that compares against its read-out
        r["call_apply_us_per_frame"] = time_events(lambda: call(r["reach_cells"], apply=1), a.reps, a.inner, F)
        print("%.2f m, reach %g m = %d cells: %.0f rays and %.0f steps per frame, %.0f miss atomics; call %.1f us / frame (with apply %.1f); zero %.1f us, apply kernel %.1f us, "
              "ray kernel %.1f us / frame = %.0f look-ups / us (numbered from 0, %d touched: %.1f us = %.0f look-ups / us); unfused %.0f us / frame (%.0fx); touched %d, carved %d of %d voxels in %d slots" % (
                  size, r["reach_m"], r["reach_cells"], r["rays_per_frame"], r["steps_per_frame"], r["miss_atomics_per_frame"], r["call_us_per_frame"]["us"],
                  r["call_apply_us_per_frame"]["us"], r["zero_us"]["us"], r["apply_kernel_us"], r["ray_kernel_us_per_frame"], r["lookups_per_us"], r["touched_numbered_from_0"], r["ray_kernel_without_atomics_us_per_frame"], r["lookups_per_us_without_atomics"],
                  r["unfused_us_per_frame"]["us"], r["unfused_over_fused"], r["touched"], r["carved"], V, slots), flush=True)
    res["sizes"].append(entry)
    del buf, miss, vkeys, vlast
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
