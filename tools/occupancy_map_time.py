#!/usr/bin/env python3
"""The world-fixed occupancy map on KITTI states (HIP events around the C entry on pre-allocated buffers, median of --reps samples, each
sample --inner calls back to back): for B = 1, 16, 256 frames fused in place into a map of 2000 x 2000 cells at scale 10 (x -40..160,
y -100..100) along a straight line with a slow turn (0.5 m and 0.002 rad per frame):
  (a) us per call and per frame of sv_occupancy_fuse_device with the cull on and off, and the per-lane lookups either way
      (sv_debug_occupancy_fuse's counter; without the cull rows x cols x B);
  (b) the form a user writes without this entry, in the same process and alternated with (a) sample by sample, after asserting that it
      yields the same map: a per-frame loop of torch index arithmetic and torch.where over the whole map.
The states are StereoRig.occupancy's (vehicle axes, the CLI's grid) of the committed KITTI frames 0 .. 6 (tests/golden), cycled to fill
the batch.

    python tools/occupancy_map_time.py [--reps 20] [--inner 5] [--out profiles/occupancy_map_time.json]
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
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--batches", default="1,16,256")
ap.add_argument("--out", default="")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
sv = importlib.import_module(PKG + ".stereo_vision.sv")
L = eng.occupancy_map_lib()
W, H = 1242, 375
G = os.path.join(ROOT, "tests", "golden")


def png(name):
    return np.asarray(Image.open(os.path.join(G, name)))


def gray3(name):
    return np.ascontiguousarray(np.repeat(png(name)[..., None], 3, -1))


ls = [png("kitti0_color_left.png")] + [gray3("kitti%d_left.png" % k) for k in range(1, 7)]
rs = [png("kitti0_color_right.png")] + [gray3("kitti%d_right.png" % k) for k in range(1, 7)]
rig = rigmod.StereoRig(W, H)
occ = rig.occupancy(torch.from_numpy(np.stack(ls)).cuda(), torch.from_numpy(np.stack(rs)).cuda(), pixel_format="rgb", transform=(sv.CAMERA_TO_VEHICLE, None),
                    **sv.CLI_TOP_VIEW)
rig.close()
states_all, frame = occ.state, occ.spec
FROWS, FCOLS = states_all.shape[1:]
MAP = dict(x_range=(-40, 160), y_range=(-100, 100), scale=10)
words = sv.occupancy_map_params(**MAP)
spec = eng.occupancy_map_spec(**MAP)
ROWS, COLS = words["rows"], words["cols"]
STEP_M, STEP_RAD = 0.5, 0.002


def drive(n):
    yaw = STEP_RAD * np.arange(n)
    x = np.concatenate([[0.0], np.cumsum(STEP_M * np.cos(yaw))[:-1]])
    y = np.concatenate([[0.0], np.cumsum(STEP_M * np.sin(yaw))[:-1]])
    return sv.occupancy_pose(x, y, yaw)


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner  # us per call


def time_alternated(fns, reps, inner):
    """{name: median us per call}; one sample of each in turn, reps times over."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(sample(fn, inner))
    return {k: float(np.median(v)) for k, v in ts.items()}


Xw_np, Yw_np = sv.occupancy_map_centres(words)
Xw, Yw = torch.from_numpy(Xw_np).cuda()[:, None], torch.from_numpy(Yw_np).cuda()[None, :]
(FX0, FX1), (FY0, FY1), FS = sv.CLI_TOP_VIEW["x_range"], sv.CLI_TOP_VIEW["y_range"], float(sv.CLI_TOP_VIEW["scale"])
FR1, FC1 = int(FX1 * FS), int(FY1 * FS)


def torch_loop(states, poses, logodds, last_seen, seq0=0):
    """The map after the frames, with torch ops over the whole map per frame; poses is a host array."""
    Lm, Sm = logodds.to(torch.int32), last_seen.clone()
    for b in range(states.shape[0]):
        tx, ty, c, s = (float(v) for v in poses[b])
        dx, dy = Xw - tx, Yw - ty
        Xf, Yf = c * dx + s * dy, c * dy - s * dx
        seen = (Xf > FX0) & (Xf < FX1) & (Yf > FY0) & (Yf < FY1)
        fr = (FR1 - torch.trunc(Xf * FS)).long().clamp_(0, FROWS - 1)
        fc = (FC1 - torch.trunc(Yf * FS)).long().clamp_(0, FCOLS - 1)
        st = torch.where(seen, states[b][fr, fc], torch.zeros((), dtype=torch.uint8, device="cuda"))
        up = torch.clamp(Lm + words["l_occ"], words["l_min"], words["l_max"])
        down = torch.clamp(Lm - words["l_free"], words["l_min"], words["l_max"])
        Lm = torch.where(st == 2, up, torch.where(st == 1, down, Lm))
        Sm = torch.where((st == 1) | (st == 2), torch.full((), seq0 + b, dtype=torch.int32, device="cuda"), Sm)
    return Lm.to(torch.int16), Sm


res = {"map": dict(rows=ROWS, cols=COLS, scale=MAP["scale"]), "frame_grid": [int(FROWS), int(FCOLS)], "step_m": STEP_M, "step_rad": STEP_RAD, "reps": a.reps,
       "inner": a.inner, "rows": []}
for B in [int(b) for b in a.batches.split(",")]:
    states = states_all[torch.arange(B) % states_all.shape[0]].contiguous()
    poses = drive(B)
    t_poses = torch.from_numpy(poses).cuda()
    logodds = torch.zeros((ROWS, COLS), dtype=torch.int16, device="cuda")
    last_seen = torch.full((ROWS, COLS), -1, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def fused():
        rc = L.sv_occupancy_fuse_device(states.data_ptr(), t_poses.data_ptr(), B, 0, ctypes.byref(frame), ctypes.byref(spec), 0, 0, logodds.data_ptr(), last_seen.data_ptr(),
                                        logodds.data_ptr(), last_seen.data_ptr(), st)
        assert rc == 0

    def loop():
        torch_loop(states, poses, logodds, last_seen)

    fused()
    torch.cuda.synchronize()
    want = torch_loop(states, poses, torch.zeros_like(logodds), torch.full_like(last_seen, -1))
    same = torch.equal(want[0], logodds) and torch.equal(want[1], last_seen)
    assert same, "the torch loop differs from the fused map"
    row = {"batch": B, "torch_loop_equals_fused": same, "cells_covered": int((last_seen >= 0).sum().item())}
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    for cull in (True, False):
        counter.zero_()
        torch.cuda.synchronize()
        eng.debug_occupancy_fuse(cull, counter)
        fused()
        torch.cuda.synchronize()
        row["lookups" + ("" if cull else "_no_cull")] = int(counter.item())
    eng.debug_occupancy_fuse(True, None)
    t = time_alternated({"fused": fused, "torch_loop": loop}, a.reps, a.inner)
    eng.debug_occupancy_fuse(False, None)
    t_off = time_alternated({"fused": fused}, a.reps, a.inner)
    eng.debug_occupancy_fuse(True, None)
    row.update({"fused_us": t["fused"], "fused_us_per_frame": t["fused"] / B, "fused_no_cull_us": t_off["fused"], "fused_no_cull_us_per_frame": t_off["fused"] / B,
                "torch_loop_us": t["torch_loop"], "torch_loop_us_per_frame": t["torch_loop"] / B, "torch_loop_over_fused": t["torch_loop"] / t["fused"],
                "no_cull_over_cull": t_off["fused"] / t["fused"], "lookups_no_cull_over_cull": row["lookups_no_cull"] / max(row["lookups"], 1)})
    res["rows"].append(row)
    print("B=%-3d fused %.1f us (%.2f us/frame; no cull %.1f us, x%.2f)  torch loop %.1f us (x%.1f)  lookups %d (no cull %d, x%.2f)  cells covered %d"
          % (B, row["fused_us"], row["fused_us_per_frame"], row["fused_no_cull_us"], row["no_cull_over_cull"], row["torch_loop_us"], row["torch_loop_over_fused"],
             row["lookups"], row["lookups_no_cull"], row["lookups_no_cull_over_cull"], row["cells_covered"]), flush=True)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
