#!/usr/bin/env python3
"""The correlative match on KITTI states (HIP events around the C entry on pre-allocated buffers, median of --reps samples, each sample
--inner calls back to back): B = 1, 16, 256 frames against a map of 2000 x 2000 cells at scale 10 (x -40..160, y -100..100) fused from them
along a straight line with a slow turn (0.5 m and 0.002 rad per frame), P = 245 (7 x 7 x 5) and 2205 (21 x 21 x 5) candidates per frame in a
window of +-0.3 m, +-0.3 m, +-0.02 rad (+-1.0 m for the larger) around the frame's pose, w_free = 0 and 1:
  (a) us per call of sv_map_match_device and of its stages (SV_MAP_MATCH_STAGE: the lists alone, lists + scores, the whole call), the map
      lookups made (sv_debug_map_match's counter) and ns per lookup;
  (b) the same call with the candidates per workgroup fixed at 1 - the candidate uniform per workgroup, its lanes striding over the list -
      and at 256, beside the call's own choice;
  (c) the form a user writes without this entry, in the same process and alternated with (a) sample by sample, after asserting that it
      yields the same sums, counts and best score: per frame nonzero cells, a broadcast [P, n] transform, index_select and a sum.
The states are StereoRig.occupancy's (vehicle axes, the CLI's grid) of the committed KITTI frames 0 .. 6 (tests/golden), cycled to fill
the batch.  For scale the fuse's cost per frame is taken from profiles/occupancy_map_time.json.

    python tools/map_match_time.py [--reps 20] [--inner 5] [--out profiles/map_match_time.json]
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
ap.add_argument("--windows", default="7x7x5,21x21x5")
ap.add_argument("--torch-max", type=int, default=16, help="the torch form is timed up to this batch (it is a per-frame loop)")
ap.add_argument("--out", default="")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
sv = importlib.import_module(PKG + ".stereo_vision.sv")
L = eng.map_match_lib()
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
ROWS, COLS, TOP, LEFT, MS = words["rows"], words["cols"], words["top"], words["left"], float(words["scale"])
STEP_M, STEP_RAD = 0.5, 0.002


def drive(n):
    yaw = STEP_RAD * np.arange(n)
    x = np.concatenate([[0.0], np.cumsum(STEP_M * np.cos(yaw))[:-1]])
    y = np.concatenate([[0.0], np.cumsum(STEP_M * np.sin(yaw))[:-1]])
    return np.stack([x, y, yaw], -1)


def sample(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner  # us per call


def time_alternated(fns, reps, inner):
    """{name: median us per call}; one sample of each in turn, reps times over.  A form whose call takes more than 5 ms is sampled one call
    at a time instead of `inner`."""
    per = {}
    for k, fn in fns.items():
        fn()
        fn()
        per[k] = inner if sample(fn, 1) < 5e3 else 1
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(sample(fn, per[k]))
    return {k: float(np.median(v)) for k, v in ts.items()}


Xp_np, Yp_np = sv.occupancy_frame_points(sv.CLI_TOP_VIEW)
Xp, Yp = torch.from_numpy(Xp_np).cuda(), torch.from_numpy(Yp_np).cuda()


def torch_form(states, poses, logodds, w_occ, w_free):
    """(sums [B,P,2], counts [B,P,2], the largest score [B]) with torch ops per frame; poses is a device tensor [B,P,4]."""
    flat = logodds.reshape(-1)
    B, P = poses.shape[:2]
    sums, counts = torch.zeros((B, P, 2), dtype=torch.int64, device="cuda"), torch.zeros((B, P, 2), dtype=torch.int32, device="cuda")
    for b in range(B):
        tx, ty, c, s = (poses[b, :, k][:, None] for k in range(4))
        for slot, byte in ((0, 2), (1, 1)):
            if byte == 1 and w_free == 0:
                continue
            fr, fc = torch.nonzero(states[b] == byte, as_tuple=True)
            Xf, Yf = Xp[fr][None, :], Yp[fc][None, :]
            Xw, Yw = (c * Xf - s * Yf) + tx, (s * Xf + c * Yf) + ty
            gx, gy = torch.floor(Xw * MS), torch.floor(Yw * MS)
            inside = (gx >= TOP - ROWS) & (gx <= TOP - 1) & (gy >= LEFT - COLS) & (gy <= LEFT - 1)
            r = (TOP - 1 - gx).clamp_(0, ROWS - 1).long()
            cc = (LEFT - 1 - gy).clamp_(0, COLS - 1).long()
            v = torch.index_select(flat, 0, (r * COLS + cc).reshape(-1)).reshape(r.shape).long()
            sums[b, :, slot] = torch.where(inside, v, torch.zeros((), dtype=torch.int64, device="cuda")).sum(1)
            counts[b, :, slot] = inside.sum(1).int()
    score = w_occ * sums[..., 0] - w_free * sums[..., 1]
    return sums, counts, score.max(1).values


fuse_us_per_frame = None
try:
    with open(os.path.join(ROOT, "profiles", "occupancy_map_time.json")) as f:
        fuse_us_per_frame = {row["batch"]: row["fused_us_per_frame"] for row in json.load(f)["rows"]}
except (OSError, KeyError, ValueError):
    pass

res = {"map": dict(rows=ROWS, cols=COLS, scale=MAP["scale"]), "frame_grid": [int(FROWS), int(FCOLS)], "step_m": STEP_M, "step_rad": STEP_RAD, "reps": a.reps,
       "inner": a.inner, "fuse_us_per_frame": fuse_us_per_frame, "rows": []}
counter = torch.zeros(1, dtype=torch.int64, device="cuda")
for B in [int(b) for b in a.batches.split(",")]:
    states = states_all[torch.arange(B) % states_all.shape[0]].contiguous()
    xyyaw = drive(B)
    logodds = eng.occupancy_fuse(states, sv.occupancy_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2]), frame, words).logodds
    for window in a.windows.split(","):
        steps = tuple(int(v) for v in window.split("x"))
        half = (0.3, 0.3, 0.02) if steps[0] <= 7 else (1.0, 1.0, 0.02)
        cand = np.stack([sv.occupancy_pose_window(x, y, yaw, half, steps) for x, y, yaw in xyyaw])
        P = cand.shape[1]
        poses = torch.from_numpy(sv.occupancy_pose(cand[..., 0], cand[..., 1], cand[..., 2])).cuda()
        for w_free in (0, 1):
            need = ctypes.c_size_t()
            assert L.sv_map_match_workspace(ctypes.byref(frame), B, w_free, ctypes.byref(need)) == 0
            ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
            sums, counts = torch.empty((B, P, 2), dtype=torch.int64, device="cuda"), torch.empty((B, P, 2), dtype=torch.int32, device="cuda")
            best, best_score = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")
            st = torch.cuda.current_stream().cuda_stream

            def fused():
                rc = L.sv_map_match_device(states.data_ptr(), poses.data_ptr(), B, P, ctypes.byref(frame), ctypes.byref(spec), logodds.data_ptr(), 1, w_free, sums.data_ptr(),
                                           counts.data_ptr(), best.data_ptr(), best_score.data_ptr(), ws.data_ptr(), need.value, st)
                assert rc == 0

            def loop():
                torch_form(states, poses, logodds, 1, w_free)

            counter.zero_()
            torch.cuda.synchronize()
            eng.debug_map_match(0, counter)
            fused()
            torch.cuda.synchronize()
            eng.debug_map_match(0, None)
            n_list = int((states == 2).sum().item()) + (int((states == 1).sum().item()) if w_free else 0)
            row = {"batch": B, "n_poses": P, "w_free": w_free, "lookups": int(counter.item()), "list_entries": n_list}
            assert row["lookups"] == n_list * P
            with_torch = B <= a.torch_max
            if with_torch:
                want = torch_form(states, poses, logodds, 1, w_free)
                same = torch.equal(want[0], sums) and torch.equal(want[1], counts) and torch.equal(want[2], best_score) and torch.equal((sums[..., 0] - w_free * sums[..., 1]).gather(1, best.long()[:, None])[:, 0], best_score)
                assert same, "the torch form differs from the fused call"
                row["torch_form_equals_fused"] = same
            t = time_alternated({"fused": fused, "torch": loop} if with_torch else {"fused": fused}, a.reps, a.inner)
            row["fused_us"], row["ns_per_lookup"] = t["fused"], t["fused"] * 1e3 / max(row["lookups"], 1)
            row["fused_us_per_frame"] = t["fused"] / B
            if with_torch:
                row["torch_us"], row["torch_over_fused"] = t["torch"], t["torch"] / t["fused"]
            for stage in ("lists", "scores"):
                os.environ["SV_MAP_MATCH_STAGE"] = stage
                row["upto_%s_us" % stage] = time_alternated({"fused": fused}, a.reps, a.inner)["fused"]
            os.environ.pop("SV_MAP_MATCH_STAGE")
            row["lists_us"], row["scores_us"], row["best_us"] = row["upto_lists_us"], row["upto_scores_us"] - row["upto_lists_us"], t["fused"] - row["upto_scores_us"]
            for group in (1, 256):
                eng.debug_map_match(group, None)
                row["group_%d_us" % group] = time_alternated({"fused": fused}, a.reps, a.inner)["fused"]
            eng.debug_map_match(0, None)
            fused()
            torch.cuda.synchronize()
            res["rows"].append(row)
            print("B=%-3d P=%-4d w_free=%d  call %.1f us (%.2f us/frame; lists %.1f, scores %.1f, best %.1f)  %.3f ns/lookup of %d  group 1: %.1f us, 256: %.1f us  torch %s"
                  % (B, P, w_free, row["fused_us"], row["fused_us_per_frame"], row["lists_us"], row["scores_us"], row["best_us"], row["ns_per_lookup"], row["lookups"],
                     row["group_1_us"], row["group_256_us"], "%.1f us (x%.1f)" % (row["torch_us"], row["torch_over_fused"]) if with_torch else "-"), flush=True)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
        for row in res["rows"]:
            f.write(" ".join("%s=%s" % (k, ("%.3f" % v) if isinstance(v, float) else v) for k, v in row.items()) + "\n")
