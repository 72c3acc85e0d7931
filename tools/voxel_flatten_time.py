#!/usr/bin/env python3
"""The voxel map flattened into an occupancy map on a KITTI drive (HIP events, median of --reps calls after warm-up, min / max beside the
median; one process).  The map is tools/voxel_render_time.py's: B = 256 frames from the rig (the engine's d1 of the committed KITTI
frames, cycled) along a gently turning trajectory, the CLI crop in vehicle axes, the frames' voxel rows with weights and colours inserted
at --size metres.  It is flattened into flat maps of 500 x 500 and 2000 x 2000 cells over the same 250 x 250 m (2 and 8 cells per metre),
with an absolute floor (mode 0) and with a local floor (mode 1) of radius 0, 2 and 8, at step 0.2 m and height 2 m:
  (a) us per call of sv_voxel_flatten_device into pre-allocated outputs;
  (b) the kernels by difference, with sv_debug_voxel_flatten's stages: clear alone, then with walk A, then with the floor, then with walk B,
      then all;
  (c) the voxels that take part per microsecond of either walk;
  (d) the unfused form on the same device with torch ops in the same run: the live entries of the table (a mask over its words - the
      read-out's rows carry no offset sums, which zq needs), the centres in float64 and the cell index, two scatter_reduce_ passes ("amin"
      for low, "amax" for seen), max_pool2d of the negated minima for the floor, index_add_ for the counts, a scatter_reduce_("amax") for
      top, and the resolve elementwise.  Before anything is timed both forms must agree on every output.
The yardstick is never the code under test.  Nothing is asserted about speed: fused_is_faster is reported.

    timeout -k 10 900 python tools/voxel_flatten_time.py [--reps 21] [--out profiles/voxel_flatten_time.json]
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
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--batch", type=int, default=256, help="frames of the drive")
ap.add_argument("--size", type=float, default=0.2)
ap.add_argument("--out", default="")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
svmod = importlib.import_module(PKG + ".stereo_vision.sv")
L, U = eng.voxel_map_lib(), eng.voxel_flatten_lib()
W, H = 1242, 375
G = os.path.join(ROOT, "tests", "golden")
XR = np.ascontiguousarray(svmod.CAMERA_TO_VEHICLE)
LO, HI = svmod.CLI_CLOUD_CROP
ROWS = {0.1: 65536, 0.2: 32768, 0.5: 8192}  # voxel size -> rows per frame of the voxel feed
X_RANGE, Y_RANGE = (-20, 230), (-120, 130)  # metres: the drive and its crop lie inside
FLATS = (("500x500", 2), ("2000x2000", 8))
RULES = (("absolute", dict(z_ref=0.0)), ("local_r0", dict(radius=0)), ("local_r2", dict(radius=2)), ("local_r8", dict(radius=8)))
FIELDS = ("logodds", "last_seen", "floor", "top", "cells", "stats")
NONE = 2 ** 31 - 1


def png(name):
    return np.asarray(Image.open(os.path.join(G, name)))


def gray3(name):
    return np.ascontiguousarray(np.repeat(png(name)[..., None], 3, -1))


ls = [png("kitti0_color_left.png")] + [gray3("kitti%d_left.png" % k) for k in (1, 2, 3, 4)]
rs = [png("kitti0_color_right.png")] + [gray3("kitti%d_right.png" % k) for k in (1, 2, 3, 4)]
rig = rigmod.StereoRig(W, H)
tl, tr = torch.from_numpy(np.stack(ls)).cuda(), torch.from_numpy(np.stack(rs)).cuda()
gl, gr, col = rig.frontend(tl, tr, pixel_format="rgb", colors=True)
d1_all, _ = rig.engine.process_device(gl, gr, want_d2=False)
d1_all, col = d1_all.clone(), col.clone()
Q = rig.Q.copy()
rig.close()
B, size = a.batch, a.size
sel = torch.arange(B) % d1_all.shape[0]
d1 = d1_all[sel].contiguous()
frame_no = np.arange(B, dtype=np.float64)
xyyaw = np.stack([0.8 * frame_no, 0.05 * frame_no, 0.002 * frame_no], -1)  # 204 m, turning by half a radian
poses_np = svmod.voxel_map_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2])
box_lo, box_hi = svmod.cli_voxel_map_box(xyyaw)
st = torch.cuda.current_stream().cuda_stream


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
        ts.append(e0.elapsed_time(e1) * 1e3)
    return {"us": float(np.median(ts)), "min_max": [float(np.min(ts)), float(np.max(ts))]}


vox = eng.voxel_cloud_from_disparity(d1, Q, size, LO, HI, colors=col[sel].contiguous(), XR=XR, capacity=ROWS[size])
assert (vox[5] >= 0).all().item(), "a frame holds more voxels than %d rows at size %g" % (ROWS[size], size)
probe = svmod.voxel_map_params(box_lo, box_hi, size, 2 ** 24)
buf = eng.voxel_map_new(probe)
eng.voxel_map_insert(buf, probe, vox[0], vox[1], vox[3], vox[5], poses_np)
n_voxels = eng.voxel_map_stats(buf)[0]
del buf
torch.cuda.empty_cache()
capacity = min(max(n_voxels + n_voxels // 8, 65536), 2 ** 26)  # voxel_map_time.py's rule
params = svmod.voxel_map_params(box_lo, box_hi, size, capacity)
spec, nbytes = eng.voxel_map_spec(params), L.sv_voxel_map_bytes(capacity)
buf = eng.voxel_map_new(params)
eng.voxel_map_insert(buf, params, vox[0], vox[1], vox[3], vox[5], poses_np)
del vox
torch.cuda.empty_cache()
slots = int(L.sv_voxel_map_slots(capacity))
table = buf[4:4 + 11 * slots].view(slots, 11)  # behind the head of 32 bytes: key, n, S[3], C[4], m, first_seq | last_seq << 32
res = {"batch": B, "size": size, "voxels_in_the_map": n_voxels, "capacity": capacity, "table_slots": slots, "map_bytes": nbytes, "x_range": X_RANGE, "y_range": Y_RANGE,
       "step_m": 0.2, "height_m": 2.0, "reps": a.reps, "runs": []}
as_t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")  # noqa: E731  (a tensor: torch divides by a Python number as a product with its reciprocal)
size_t, half_t, unit_t = as_t(size), as_t(0.5), as_t(65536.0)
lo_t = [as_t(v) for v in params["lo"]]

for flat_name, scale in FLATS:
    flat = svmod.occupancy_map_params(X_RANGE, Y_RANGE, scale)
    rows, cols = flat["rows"], flat["cols"]
    flat_c = eng._occupancy_map_struct(flat)
    ms_t = as_t(float(scale))
    for rule_name, rule in RULES:
        words = svmod.voxel_flatten_params(params, **rule)
        fspec = eng.voxel_flatten_spec(words)
        out = eng.voxel_map_flatten(buf, params, flat, words)

        def call():
            rc = U.sv_voxel_flatten_device(buf.data_ptr(), nbytes, ctypes.byref(spec), ctypes.byref(flat_c), ctypes.byref(fspec), 1, 1, 0, out.logodds.data_ptr(),
                                           out.last_seen.data_ptr(), out.floor.data_ptr(), out.top.data_ptr(), out.cells.data_ptr(), out.stats.data_ptr(), st)
            assert rc == 0, L.sv_last_error(None)

        def unfused():
            key, n = table[:, 0], table[:, 1]
            live = ((key != -1) & (n >= 1) & (table[:, 9] >= 1) & ((table[:, 10] >> 32) >= 0)).nonzero(as_tuple=True)[0]
            e = table[live]
            key, n, nf, last = e[:, 0], e[:, 1], e[:, 1].double(), e[:, 10] >> 32
            g = [torch.floor((lo_t[k] + (((key >> (20 * k)) & 0xFFFFF).double() + (e[:, 2 + k].double() + half_t * nf) / (unit_t * nf)) * size_t) * ms_t) for k in range(2)]
            inside = (g[0] >= flat["top"] - rows) & (g[0] <= flat["top"] - 1) & (g[1] >= flat["left"] - cols) & (g[1] <= flat["left"] - 1)
            stats = torch.zeros(8, dtype=torch.int64, device="cuda")
            stats[0], stats[1] = inside.sum(), (~inside).sum()
            at = inside.nonzero(as_tuple=True)[0]
            cell = (flat["top"] - 1 - g[0][at].long()) * cols + (flat["left"] - 1 - g[1][at].long())
            zq = ((key[at] >> 40) & 0xFFFFF) * 256 + (torch.div(e[at, 4], n[at], rounding_mode="floor") >> 8)
            low = torch.full((rows * cols,), NONE, dtype=torch.int64, device="cuda").scatter_reduce_(0, cell, zq, "amin")
            seen = torch.full((rows * cols,), -1, dtype=torch.int64, device="cuda").scatter_reduce_(0, cell, last[at], "amax")
            if words["mode"] == 0:
                base = torch.full_like(low, words["z_ref_q"])
                floor = base
            else:
                R = words["radius"]
                base = low if R == 0 else (-torch.nn.functional.max_pool2d((-low).double().view(1, 1, rows, cols), 2 * R + 1, stride=1, padding=R)).long().view(-1)
                floor = torch.where(base == NONE, torch.full_like(base, -1), base)
            h = zq - base[cell]
            kind = torch.where(h < -words["step_q"], 0, torch.where(h < words["step_q"], 1, torch.where(h < words["height_q"], 2, 3)))
            counted = kind > 0
            counts = torch.zeros(rows * cols * 3, dtype=torch.int64, device="cuda").index_add_(0, cell[counted] * 3 + kind[counted] - 1, torch.ones_like(cell[counted]))
            counts = counts.view(-1, 3)
            solid = (kind == 1) | (kind == 2)
            top = torch.full((rows * cols,), -1, dtype=torch.int64, device="cuda").scatter_reduce_(0, cell[solid], zq[solid], "amax")
            occupied = counts[:, 1] >= words["min_obstacle"]
            free = ~occupied & (counts[:, 0] >= words["min_ground"])
            Lw = torch.where(occupied, (counts[:, 1] * flat["l_occ"]).clamp(max=flat["l_max"]), torch.where(free, (-(counts[:, 0] * flat["l_free"])).clamp(min=flat["l_min"]), 0))
            stats[2:6] = torch.bincount(kind, minlength=4)
            stats[6], stats[7] = occupied.sum(), free.sum()
            return {"logodds": Lw.to(torch.int16).view(rows, cols), "last_seen": torch.where(occupied | free, seen, -1).int().view(rows, cols), "floor": floor.int().view(rows, cols),
                    "top": top.int().view(rows, cols), "cells": counts.int().view(rows, cols, 3), "stats": stats}

        call()
        slow = unfused()
        torch.cuda.synchronize()
        for k in FIELDS:
            assert torch.equal(getattr(out, k), slow[k]), "the fused and the unfused form disagree on %s at %s, %s" % (k, flat_name, rule_name)
        stats = out.stats.cpu().tolist()
        entry = {"flat": flat_name, "scale": scale, "rule": rule_name, "words": words, "stats": dict(zip(svmod.VOXEL_FLATTEN_STATS, stats))}
        stages = {}
        for k, name in ((1, "clear"), (2, "clear_a"), (3, "clear_a_floor"), (4, "clear_a_floor_b"), (0, "call")):
            eng.debug_voxel_flatten(0, k)
            stages[name] = time_events(call, a.reps)
        eng.debug_voxel_flatten(0, 0)
        call()
        took = stats[0] + stats[1]  # the voxels that pass the filters: what either walk computes a cell for
        entry["call_us"] = stages["call"]
        entry["clear_kernel_us"] = stages["clear"]["us"]
        entry["walk_a_kernel_us"] = stages["clear_a"]["us"] - stages["clear"]["us"]
        entry["floor_kernel_us"] = stages["clear_a_floor"]["us"] - stages["clear_a"]["us"]
        entry["walk_b_kernel_us"] = stages["clear_a_floor_b"]["us"] - stages["clear_a_floor"]["us"]
        entry["resolve_kernel_us"] = stages["call"]["us"] - stages["clear_a_floor_b"]["us"]
        entry["walk_a_voxels_per_us"] = took / entry["walk_a_kernel_us"]
        entry["walk_b_voxels_per_us"] = took / entry["walk_b_kernel_us"]
        entry["unfused_us"] = time_events(unfused, max(a.reps // 2, 5))
        entry["unfused_over_fused"] = entry["unfused_us"]["us"] / stages["call"]["us"]
        entry["fused_is_faster"] = bool(entry["unfused_over_fused"] > 1)
        print("%s %s: %d voxels, %d drawn; call %.1f us (clear %.1f, walk A %.1f, floor %.1f, walk B %.1f, resolve %.1f) = %.0f and %.0f voxels / us; unfused %.0f us (%.1fx)"
              % (flat_name, rule_name, n_voxels, stats[0], stages["call"]["us"], entry["clear_kernel_us"], entry["walk_a_kernel_us"], entry["floor_kernel_us"], entry["walk_b_kernel_us"],
                 entry["resolve_kernel_us"], entry["walk_a_voxels_per_us"], entry["walk_b_voxels_per_us"], entry["unfused_us"]["us"], entry["unfused_over_fused"]), flush=True)
        res["runs"].append(entry)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
