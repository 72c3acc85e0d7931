#!/usr/bin/env python3
"""The clearance field of the world map and the path check on a KITTI map (HIP events around the C entries on pre-allocated buffers, median
of --reps samples, each sample --inner calls back to back).  The map is occupancy_map_time.py's: 2000 x 2000 cells at scale 10 (x -40..160,
y -100..100), fused from the committed KITTI frames 0 .. 6 (tests/golden) along that tool's drive (0.5 m and 0.002 rad per frame).
  (a) sv_clearance_device for R in 10, 50, 254 cells, sources = occupied cells (unknown 0) and occupied or never-seen cells (unknown 1):
      us per call with the early exit (the call), without it (sv_debug_clearance's variant 3), of each pass alone (SV_CLEARANCE_PASS), of the
      fused kernel where R <= 32 (variant 1), and the row walk's taps against rows x cols x (2 R + 1);
  (b) sv_clearance_paths_device for K = 256 and 4096 paths of 64 steps and 3 discs against the field of R = 10;
  (c) the form a user writes without these entries, in the same process and alternated with (a) / (b) sample by sample, after asserting that
      it yields the same bits: 2 R + 1 shifted torch.minimum per pass over the whole map, and a broadcast transform + index_select + amin.
profiles/occupancy_map_time.json's fuse at B = 1 is quoted for scale: both calls move the same map once.

    python tools/clearance_time.py [--reps 20] [--inner 5] [--out profiles/clearance_time.json]
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
ap.add_argument("--radii", default="10,50,254")
ap.add_argument("--paths", default="256,4096")
ap.add_argument("--out", default="")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
sv = importlib.import_module(PKG + ".stereo_vision.sv")
L = eng.clearance_lib()
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
MAP = dict(x_range=(-40, 160), y_range=(-100, 100), scale=10)
STEP_M, STEP_RAD = 0.5, 0.002


def drive(n):
    yaw = STEP_RAD * np.arange(n)
    x = np.concatenate([[0.0], np.cumsum(STEP_M * np.cos(yaw))[:-1]])
    y = np.concatenate([[0.0], np.cumsum(STEP_M * np.sin(yaw))[:-1]])
    return sv.occupancy_pose(x, y, yaw)


world = rigmod.OccupancyMap(**MAP)
world.update(occ, drive(7))
words, spec = world.words, eng._occupancy_map_struct(world.words)
ROWS, COLS, T_OCC = words["rows"], words["cols"], words["l_occ"]
logodds, last_seen = world.logodds, world.last_seen
d2 = torch.empty((ROWS, COLS), dtype=torch.int16, device="cuda")  # the uint16 field's bits: torch has few operators for uint16
ws = torch.empty(ROWS * COLS, dtype=torch.uint8, device="cuda")
STREAM = torch.cuda.current_stream().cuda_stream


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


def as_int32(t16):
    """The values of a uint16 field kept in an int16 tensor, as int32."""
    return t16.to(torch.int32) & 0xFFFF


def torch_field(R, unknown):
    """int32 [rows,cols]: the field with 2 R + 1 shifted minima per pass over the whole map."""
    src = logodds >= T_OCC
    if unknown:
        src = src | (last_seen < 0)
    none = torch.full((), 255, dtype=torch.int32, device="cuda")
    g = torch.where(src, torch.zeros((), dtype=torch.int32, device="cuda"), none)
    for dr in range(1, min(R, ROWS - 1) + 1):
        cand = torch.where(src, torch.full((), dr, dtype=torch.int32, device="cuda"), none)
        g[dr:] = torch.minimum(g[dr:], cand[:-dr])
        g[:-dr] = torch.minimum(g[:-dr], cand[dr:])
    g2 = g * g
    best = g2.clone()
    for dc in range(1, min(R, COLS - 1) + 1):
        best[:, dc:] = torch.minimum(best[:, dc:], g2[:, :-dc] + dc * dc)
        best[:, :-dc] = torch.minimum(best[:, :-dc], g2[:, dc:] + dc * dc)
    return torch.where(best > R * R, torch.full((), 65535, dtype=torch.int32, device="cuda"), best)


def field_call(R, unknown):
    rc = L.sv_clearance_device(logodds.data_ptr(), last_seen.data_ptr(), ROWS, COLS, R, T_OCC, unknown, d2.data_ptr(), ws.data_ptr(), ws.numel(), STREAM)
    assert rc == 0, L.sv_last_error(None)


def with_pass(name, fn):
    """fn with SV_CLEARANCE_PASS = name around it."""
    def run():
        os.environ["SV_CLEARANCE_PASS"] = name
        try:
            fn()
        finally:
            del os.environ["SV_CLEARANCE_PASS"]
    return run


fuse_us = None
try:
    with open(os.path.join(ROOT, "profiles", "occupancy_map_time.json")) as f:
        fuse_us = [r["fused_us"] for r in json.load(f)["rows"] if r["batch"] == 1][0]
except (OSError, KeyError, IndexError, ValueError):
    pass
res = {"map": dict(rows=ROWS, cols=COLS, scale=MAP["scale"]), "t_occ": T_OCC, "occupied_cells": int((logodds >= T_OCC).sum().item()),
       "never_seen_cells": int((last_seen < 0).sum().item()), "reps": a.reps, "inner": a.inner, "fuse_b1_us_from_occupancy_map_time": fuse_us, "field": [], "paths": []}
print("map %d x %d: %d occupied cells, %d never seen; one fuse call at B = 1: %s us" % (ROWS, COLS, res["occupied_cells"], res["never_seen_cells"], fuse_us), flush=True)
counter = torch.zeros(1, dtype=torch.int64, device="cuda")
fields = {}
for R in [int(v) for v in a.radii.split(",")]:
    for unknown in (0, 1):
        call = lambda: field_call(R, unknown)  # noqa: E731
        want = torch_field(R, unknown)
        row = {"radius": R, "unknown": unknown, "taps_full": ROWS * COLS * (2 * R + 1)}
        variants = [("", 0), ("_no_exit", 3)] + ([("_fused", 1)] if R <= 32 else [])
        for name, variant in variants:
            counter.zero_()
            d2.zero_()
            torch.cuda.synchronize()
            eng.debug_clearance(variant, counter)
            call()
            torch.cuda.synchronize()
            eng.debug_clearance(0, None)
            same = torch.equal(as_int32(d2), want)
            assert same, "the torch form differs from the kernels at R = %d, unknown = %d, variant %d" % (R, unknown, variant)
            row["taps" + name] = int(counter.item())
        assert row["taps_no_exit"] == row["taps_full"]
        row["torch_equals_kernels"] = True
        if R == 10 and unknown == 0:
            fields[R] = d2.clone()
        reps_torch = a.reps if R <= 50 else max(3, a.reps // 4)
        t = time_alternated({"call": call, "torch": lambda: torch_field(R, unknown)}, reps_torch, a.inner if R <= 50 else 1)
        t.update(time_alternated({"call": call, "cols": with_pass("cols", call), "rows": with_pass("rows", call)}, a.reps, a.inner))
        for name, variant in variants[1:]:
            eng.debug_clearance(variant, None)
            t["call" + name] = time_alternated({"call": call}, a.reps, a.inner)["call"]
            eng.debug_clearance(0, None)
        row.update({"call_us": t["call"], "cols_us": t["cols"], "rows_us": t["rows"], "no_exit_us": t["call_no_exit"], "fused_kernel_us": t.get("call_fused"),
                    "torch_us": t["torch"], "torch_over_call": t["torch"] / t["call"], "taps_over_full": row["taps"] / row["taps_full"],
                    "no_exit_over_call": t["call_no_exit"] / t["call"], "call_over_fuse_b1": None if fuse_us is None else t["call"] / fuse_us})
        res["field"].append(row)
        print("R=%-3d unknown=%d call %.1f us (cols %.1f, rows %.1f; no exit %.1f, x%.2f; fused kernel %s)  torch %.1f us (x%.1f)  taps %d of %d (%.4f)  vs fuse x%s"
              % (R, unknown, row["call_us"], row["cols_us"], row["rows_us"], row["no_exit_us"], row["no_exit_over_call"],
                 "-" if row["fused_kernel_us"] is None else "%.1f us" % row["fused_kernel_us"], row["torch_us"], row["torch_over_call"], row["taps"], row["taps_full"],
                 row["taps_over_full"], "-" if fuse_us is None else "%.2f" % row["call_over_fuse_b1"]), flush=True)

# ---- paths against the field of R = 10 with occupied cells as sources
R, T, TOP, LEFT, MS = 10, 64, words["top"], words["left"], float(words["scale"])
field = fields.get(R)
if field is None:
    field_call(R, 0)
    field = d2.clone()
field32 = as_int32(field).reshape(-1)
centres, r2 = sv.clearance_discs([(0.0, 0.0, 0.9), (1.3, 0.0, 0.9), (2.6, 0.0, 0.9)], MAP["scale"])
t_centres, t_r2 = torch.from_numpy(centres).cuda(), torch.from_numpy(r2).cuda()
steps = torch.arange(T, dtype=torch.int32, device="cuda")


def torch_paths(poses):
    p = poses[:, :, None, :]
    tx, ty, c, s = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    px, py = t_centres[:, 0], t_centres[:, 1]
    gx, gy = torch.floor(((c * px - s * py) + tx) * MS), torch.floor(((s * px + c * py) + ty) * MS)
    inside = (gx >= TOP - ROWS) & (gx <= TOP - 1) & (gy >= LEFT - COLS) & (gy <= LEFT - 1)
    r, cc = (TOP - 1 - gx).long().clamp_(0, ROWS - 1), (LEFT - 1 - gy).long().clamp_(0, COLS - 1)
    v = field32.index_select(0, (r * COLS + cc).reshape(-1)).reshape(inside.shape)
    v = torch.where(inside, v, torch.full((), 65535, dtype=torch.int32, device="cuda"))
    hit = (inside & (v <= t_r2)).any(2)
    first = torch.where(hit, steps, torch.full((), T, dtype=torch.int32, device="cuda")).amin(1)
    return first, v.amin((1, 2)), (~inside).sum((1, 2)).to(torch.int32)


for K in [int(v) for v in a.paths.split(",")]:
    bend = np.linspace(-1.0, 1.0, K)[:, None]
    s_ = np.linspace(0.0, 1.0, T)[None, :]
    reach = 20.0 + 100.0 * (np.arange(K) % 7 / 6.0)[:, None]  # the longest leave the map at its far end
    yaw = bend * s_
    poses = torch.from_numpy(sv.occupancy_pose(reach * s_ * np.cos(yaw), reach * s_ * np.sin(yaw), yaw)).cuda()
    outs = [torch.empty(K, dtype=torch.int32, device="cuda") for _ in range(3)]

    def call():
        rc = L.sv_clearance_paths_device(field.data_ptr(), ctypes.byref(spec), poses.data_ptr(), K, T, centres.ctypes.data, r2.ctypes.data, len(r2), R,
                                         outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), STREAM)
        assert rc == 0, L.sv_last_error(None)

    call()
    torch.cuda.synchronize()
    want = torch_paths(poses)
    assert all(torch.equal(o, w) for o, w in zip(outs, want)), "the torch form differs from the path kernel at K = %d" % K
    t = time_alternated({"call": call, "torch": lambda: torch_paths(poses)}, a.reps, a.inner)
    row = {"paths": K, "steps": T, "discs": len(r2), "torch_equals_kernel": True, "paths_hit": int((outs[0] < T).sum().item()), "paths_outside": int((outs[2] > 0).sum().item()),
           "call_us": t["call"], "torch_us": t["torch"], "torch_over_call": t["torch"] / t["call"]}
    res["paths"].append(row)
    print("K=%-4d T=%d discs=%d call %.1f us  torch %.1f us (x%.1f)  %d paths hit, %d leave the map" % (K, T, len(r2), row["call_us"], row["torch_us"], row["torch_over_call"],
                                                                                                      row["paths_hit"], row["paths_outside"]), flush=True)

if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
