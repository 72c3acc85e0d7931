#!/usr/bin/env python3
"""Voxel-grid downsampled clouds on KITTI maps (HIP events, median of --reps samples, each sample --inner calls back to back; min / max
beside the median).  B = 256 maps from the rig (the engine's d1 of the committed KITTI frames, repeated), the CLI crop in vehicle axes,
float32 with colours, voxel sizes 0.05 / 0.1 / 0.2 / 0.5 m.  Per size:
  (a) us per pair of the fused call on pre-allocated buffers and of its stages - the call is cut short behind a stage with
      SV_VOXEL_STAGE (clear, insert, mark, scan), a stage's time is the difference of two such runs;
  (b) the wavefront merge of the insert kernel on / off (sv_debug_voxel): the time, and in an untimed run the table updates and atomic
      instructions issued against the kept points;
  (c) the unfused form on the same inputs: compact_cloud_from_disparity(dtype="f64", want_index=True) and then torch device ops - cell
      keys, unique, index_add sums, the means.  It allocates inside the timed window and torch.unique reads a size back, as any user
      of it would; HIP events on the same stream span all of it.  Before anything is timed both forms must agree on every frame's set
      of cells and on the points per cell;
  (d) bytes written per pair (rows of 12 + 4 + 4 bytes) against (F)'s list for the same crop (16 bytes per kept point), and the
      workspace per pair for the capacity used.
Nothing is hidden: a size at which the fused call is not faster is reported as such ("fused_is_faster": false).

    timeout -k 10 900 python tools/voxel_cloud_time.py [--reps 10] [--inner 3] [--out profiles/voxel_cloud_time.json] [--history profiles/HISTORY.md]
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--out", default="")
ap.add_argument("--history", default="", help="append a summary of this run to this markdown file")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
svmod = importlib.import_module(PKG + ".stereo_vision.sv")
L = eng.voxel_lib()
W, H = 1242, 375
G = os.path.join(ROOT, "tests", "golden")
XR = np.ascontiguousarray(svmod.CAMERA_TO_VEHICLE)
LO, HI = svmod.CLI_CLOUD_CROP
SIZES = {0.05: 131072, 0.1: 65536, 0.2: 32768, 0.5: 8192}  # voxel size -> rows per pair
STAGES = ("clear", "insert", "mark", "scan", "write")


def png(name):
    return np.asarray(Image.open(os.path.join(G, name)))


def gray3(name):
    return np.ascontiguousarray(np.repeat(png(name)[..., None], 3, -1))


ls = [png("kitti0_color_left.png")] + [gray3("kitti%d_left.png" % k) for k in (1, 2, 3, 4)]
rs = [png("kitti0_color_right.png")] + [gray3("kitti%d_right.png" % k) for k in (1, 2, 3, 4)]
rig = rigmod.StereoRig(W, H)
tl, tr = torch.from_numpy(np.stack(ls)).cuda(), torch.from_numpy(np.stack(rs)).cuda()
d1_all = rig.disparity(tl, tr, pixel_format="rgb")
col_all = rig.frontend(tl, tr, pixel_format="rgb", colors=True)[2]
Q = rig.Q.copy()
q = np.ascontiguousarray(Q, np.float64).reshape(16)
rig.close()
B = a.batch
sel = torch.arange(B) % d1_all.shape[0]
d1, colors = d1_all[sel].contiguous(), col_all[sel].contiguous()
lo_t, hi_t = torch.tensor(LO, dtype=torch.float64, device="cuda"), torch.tensor(HI, dtype=torch.float64, device="cuda")


def time_events(fn, reps, inner):
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
        ts.append(e0.elapsed_time(e1) * 1e3 / inner / B)  # us per pair
    return {"us_per_pair": float(np.median(ts)), "min_max": [float(np.min(ts)), float(np.max(ts))]}


def fused_call(size, cap):
    """A closure that enqueues the C entry on pre-allocated outputs and workspace (no allocation in the timed window)."""
    spec = eng.voxel_spec(size, LO, HI)
    xyz = torch.empty((B, cap, 3), dtype=torch.float32, device="cuda")
    color = torch.empty((B, cap, 4), dtype=torch.uint8, device="cuda")
    cell = torch.empty((B, cap, 3), dtype=torch.int32, device="cuda")
    n = torch.empty((B, cap), dtype=torch.int32, device="cuda")
    counts = torch.empty((B,), dtype=torch.int32, device="cuda")
    nbytes = L.sv_voxel_workspace_bytes(ctypes.byref(spec), B, W, H, cap)
    ws = torch.empty((nbytes // 16 + 1, 2), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def fn(with_cell=False):
        rc = L.sv_voxel_disparity_device(d1.data_ptr(), colors.data_ptr(), B, W, H, q.ctypes.data, XR.ctypes.data, None, ctypes.byref(spec), cap,
                                         xyz.data_ptr(), color.data_ptr(), cell.data_ptr() if with_cell else None, n.data_ptr(), None, counts.data_ptr(),
                                         ws.data_ptr(), nbytes, st)
        assert rc == 0, L.sv_last_error(None)

    return fn, (xyz, color, cell, n, counts), nbytes


def unfused(size, cells):
    """(F)'s list, then torch: -> (keys of the occupied cells with the frame folded in, points per cell, centroids f32, mean colours u8)."""
    xyz, col, idx, counts = eng.compact_cloud_from_disparity(d1, Q, colors=colors, XR=XR, lo=LO, hi=HI, dtype="f64", want_index=True, capacity=CAP_F)
    valid = torch.arange(xyz.shape[1], device="cuda")[None] < counts[:, None]
    P, C = xyz[valid], col[valid]
    frame = torch.arange(B, device="cuda")[:, None].expand(B, xyz.shape[1])[valid]
    c = torch.minimum(((P - lo_t) / size).long(), cells - 1)
    key = ((frame * cells[2] + c[:, 2]) * cells[1] + c[:, 1]) * cells[0] + c[:, 0]
    uniq, inverse, n = torch.unique(key, return_inverse=True, return_counts=True)
    sums = torch.zeros((len(uniq), 3), dtype=torch.float64, device="cuda").index_add_(0, inverse, P)
    csum = torch.zeros((len(uniq), 4), dtype=torch.int64, device="cuda").index_add_(0, inverse, C.long())
    return uniq, n, (sums / n[:, None]).float(), ((2 * csum + n[:, None]) // (2 * n[:, None])).to(torch.uint8)


kept = eng.compact_cloud_from_disparity(d1, Q, XR=XR, lo=LO, hi=HI, capacity=1)[3]  # capacity 1: counts alone matter
CAP_F = int(kept.max().item())
kept_per_pair = float(kept.sum().item()) / B
res = {"width": W, "height": H, "batch": B, "disparity": "d1", "dtype": "f32", "colors": True, "transform": "CAMERA_TO_VEHICLE", "crop": [list(LO), list(HI)],
       "reps": a.reps, "inner": a.inner, "kept_points_per_pair": kept_per_pair, "compact_cloud_bytes_per_pair": 16 * kept_per_pair, "sizes": []}
for size, cap in SIZES.items():
    fn, (xyz, color, cell, n, counts), ws_bytes = fused_call(size, cap)
    cells = torch.tensor(svmod.voxel_grid(size, LO, HI)[3], device="cuda")
    # agreement first: every frame's set of cells and the points per cell
    os.environ.pop("SV_VOXEL_STAGE", None)
    fn(with_cell=True)
    torch.cuda.synchronize()
    k = counts.cpu()
    assert (k >= 0).all().item(), "a frame holds more voxels than the capacity %d at size %g" % (cap, size)
    rows = torch.arange(cap, device="cuda")[None] < counts[:, None]
    fc, fnum = cell[rows].long(), n[rows].long()
    frame = torch.arange(B, device="cuda")[:, None].expand(B, cap)[rows]
    fkey = ((frame * cells[2] + fc[:, 2]) * cells[1] + fc[:, 1]) * cells[0] + fc[:, 0]
    order = torch.argsort(fkey)
    uniq, un, umean, ucol = unfused(size, cells)
    assert torch.equal(fkey[order], uniq) and torch.equal(fnum[order], un), "the fused and the unfused form disagree at size %g" % size
    worst = (xyz[rows][order].double() - umean.double()).abs().max().item()  # float32 of two means that differ by <= size * 2^-17 + rounding
    colour_off = (color[rows][order].int() - ucol.int()).abs().max().item()
    voxels = float(k.sum().item()) / B
    del rows, fc, fnum, frame, fkey, order, uniq, un, umean, ucol
    torch.cuda.empty_cache()
    row = {"size": size, "capacity": cap, "voxels_per_pair": voxels, "points_per_voxel": kept_per_pair / voxels, "identical_cells_and_counts": True,
           "centroid_max_abs_difference_m": worst, "colour_max_difference": colour_off, "workspace_bytes_per_pair": ws_bytes / B,
           "table_slots": int(L.sv_voxel_table_slots(cap)), "bytes_written_per_pair": 20 * voxels, "bytes_written_vs_compact": 20 * voxels / (16 * kept_per_pair)}
    # (a) the whole call and its stages
    upto = {}
    for stage in STAGES:
        if stage == "write":
            os.environ.pop("SV_VOXEL_STAGE", None)
        else:
            os.environ["SV_VOXEL_STAGE"] = stage
        upto[stage] = time_events(fn, a.reps, a.inner)
    os.environ.pop("SV_VOXEL_STAGE", None)
    row["fused"] = upto["write"]
    row["stages_us_per_pair"] = {s: upto[s]["us_per_pair"] - (upto[STAGES[i - 1]]["us_per_pair"] if i else 0.0) for i, s in enumerate(STAGES)}
    # (b) the merge on / off
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    hook = {}
    for combine in (True, False):
        counters.zero_()
        eng.debug_voxel(combine, counters)
        fn()
        torch.cuda.synchronize()
        issued = counters.cpu().tolist()
        eng.debug_voxel(combine, None)
        hook["on" if combine else "off"] = dict(time_events(fn, a.reps, a.inner), table_updates_per_pair=issued[0] / B, atomic_instructions_per_pair=issued[1] / B)
    eng.debug_voxel(True, None)
    row["combine"] = hook
    # (c) the unfused form
    row["unfused"] = time_events(lambda: unfused(size, cells), max(a.reps // 2, 3), 1)
    row["unfused_over_fused"] = row["unfused"]["us_per_pair"] / row["fused"]["us_per_pair"]
    row["fused_is_faster"] = bool(row["fused"]["us_per_pair"] < row["unfused"]["us_per_pair"])
    res["sizes"].append(row)
    print("size %.2f m: %.0f voxels / pair (%.1f points each), fused %.2f us / pair [%.2f %.2f], stages %s, merge off %.2f us, updates %.0f / %.0f of %.0f "
          "points, atomics %.0f / %.0f, unfused %.1f us / pair (%.1fx), workspace %.1f MB / pair, written %.0f B (%.3f of the list)" % (
              size, voxels, row["points_per_voxel"], row["fused"]["us_per_pair"], *row["fused"]["min_max"],
              " ".join("%s %.2f" % (s, v) for s, v in row["stages_us_per_pair"].items()), hook["off"]["us_per_pair"], hook["on"]["table_updates_per_pair"],
              hook["off"]["table_updates_per_pair"], kept_per_pair, hook["on"]["atomic_instructions_per_pair"], hook["off"]["atomic_instructions_per_pair"],
              row["unfused"]["us_per_pair"], row["unfused_over_fused"], ws_bytes / B / 1e6, row["bytes_written_per_pair"], row["bytes_written_vs_compact"]), flush=True)
    del xyz, color, cell, n, counts
    torch.cuda.empty_cache()

# (F) itself on the same crop, for scale: the list the voxel form never writes
spec_f = eng.cloud_spec(lo=LO, hi=HI)
f_xyz = torch.empty((B, CAP_F, 3), dtype=torch.float32, device="cuda")
f_col = torch.empty((B, CAP_F, 4), dtype=torch.uint8, device="cuda")
f_n = torch.empty((B,), dtype=torch.int32, device="cuda")
f_bytes = L.sv_cloud_workspace_bytes(ctypes.byref(spec_f), B, W, H)
f_ws = torch.empty((f_bytes // 4,), dtype=torch.int32, device="cuda")


def compact():
    assert L.sv_cloud_disparity_device(d1.data_ptr(), colors.data_ptr(), B, W, H, q.ctypes.data, XR.ctypes.data, None, ctypes.byref(spec_f), CAP_F, f_xyz.data_ptr(),
                                       f_col.data_ptr(), None, f_n.data_ptr(), f_ws.data_ptr(), f_bytes, torch.cuda.current_stream().cuda_stream) == 0


res["compact_cloud"] = time_events(compact, a.reps, a.inner)
print("compact cloud (F), same crop, f32 with colours: %.2f us / pair, %.0f points = %.0f B / pair" % (res["compact_cloud"]["us_per_pair"], kept_per_pair, 16 * kept_per_pair))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
if a.history:
    with open(a.history, "a") as f:
        f.write("\n## Voxel-grid downsampled clouds (`tools/voxel_cloud_time.py`, `profiles/voxel_cloud_time.json`)\n\n")
        for r in res["sizes"]:
            f.write("* %.2f m, B = %d: %.0f voxels per pair; fused %.2f us per pair (%s), merge off %.2f us; table updates %.0f with / %.0f without the "
                    "merge; unfused (compact cloud f64 + torch unique / index_add) %.1f us per pair: %.1fx%s.\n" % (
                        r["size"], B, r["voxels_per_pair"], r["fused"]["us_per_pair"], ", ".join("%s %.2f" % kv for kv in r["stages_us_per_pair"].items()),
                        r["combine"]["off"]["us_per_pair"], r["combine"]["on"]["table_updates_per_pair"], r["combine"]["off"]["table_updates_per_pair"],
                        r["unfused"]["us_per_pair"], r["unfused_over_fused"], "" if r["fused_is_faster"] else " - the fused call is SLOWER here"))
        f.write("* (F) on the same crop: %.2f us per pair for %.0f points.\n" % (res["compact_cloud"]["us_per_pair"], kept_per_pair))
