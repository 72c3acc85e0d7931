#!/usr/bin/env python3
"""Compact coloured point clouds on KITTI maps (HIP events, median of --reps samples, each sample --inner calls back to back; min / max
beside the median):
  (a) us per pair of the fused disparity -> compact cloud call (count, scan, write: three kernels) on the rig's float disparity ("d1") at
      B = 1, 16, 256: no crop / the CLI crop in vehicle axes, step 1 / 4, float32 / float64, with / without colours; the kept share of the
      visited pixels per row; beside it the same call with capacity 0 (count and scan alone), which splits the time between the passes;
  (d) per row the call's own byte count - the disparity of the visited pixels read twice (count and write pass), 4 colour bytes read and
      16 or 28 bytes (12 or 24 without colours) written per kept point - over its time, as a fraction of the 8 TB/s of HBM;
  (b) the comparison with what the batch API offered before the fused call, at B = 256, CLI crop, vehicle axes, the driver's cloud
      ("dmap"), float32, colours: reproject() to the dense f64 cloud, then torch's mask, crop, boolean indexing, .float() and colour
      gather - identical results, asserted before timing -, alternated with the fused call, wall clock around a device synchronise;
  (c) rig.compact_clouds against rig.disparity, pairs/s at B = 64 on device-resident BGR frames, alternated.
The maps are the engine's d1 of the committed KITTI frames (tests/golden), repeated to fill the batch.

    python tools/compact_cloud_time.py [--reps 20] [--inner 5] [--out profiles/compact_cloud_time.json] [--history profiles/HISTORY.md]
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
ap.add_argument("--history", default="", help="append a summary of this run to this markdown file")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
svmod = importlib.import_module(PKG + ".stereo_vision.sv")
L = eng.cloud_lib()
W, H = 1242, 375
HBM_BYTES_PER_S = 8e12
G = os.path.join(ROOT, "tests", "golden")
XR = np.ascontiguousarray(svmod.CAMERA_TO_VEHICLE)
CLI_LO, CLI_HI = svmod.CLI_CLOUD_CROP


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
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def fused_call(d1, colors, crop, step, dtype, disparity="d1"):
    """A closure that enqueues the C entry on pre-allocated outputs and workspace (no allocation in the timed window)."""
    B = d1.shape[0]
    spec = eng.cloud_spec(lo=CLI_LO if crop else None, hi=CLI_HI if crop else None, step=step, disparity=disparity, dtype=dtype)
    cap = -(-W // step) * -(-H // step)
    xyz = torch.empty((B, cap, 3), dtype=torch.float32 if dtype == "f32" else torch.float64, device="cuda")
    color = torch.empty((B, cap, 4), dtype=torch.uint8, device="cuda") if colors is not None else None
    counts = torch.empty((B,), dtype=torch.int32, device="cuda")
    nbytes = L.sv_cloud_workspace_bytes(ctypes.byref(spec), B, W, H)
    ws = torch.empty((nbytes // 4,), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def fn():
        rc = L.sv_cloud_disparity_device(d1.data_ptr(), colors.data_ptr() if colors is not None else None, B, W, H, q.ctypes.data, XR.ctypes.data, None,
                                         ctypes.byref(spec), cap, xyz.data_ptr(), color.data_ptr() if color is not None else None, None, counts.data_ptr(),
                                         ws.data_ptr(), nbytes, st)
        assert rc == 0

    def count_only():  # capacity 0: the count and scan kernels alone
        rc = L.sv_cloud_disparity_device(d1.data_ptr(), None, B, W, H, q.ctypes.data, XR.ctypes.data, None, ctypes.byref(spec), 0, None, None, None,
                                         counts.data_ptr(), ws.data_ptr(), nbytes, st)
        assert rc == 0

    return fn, count_only, xyz, color, counts, cap


res = {"width": W, "height": H, "disparity": "d1", "transform": "CAMERA_TO_VEHICLE", "cli_crop": [list(CLI_LO), list(CLI_HI)], "tile": eng.cloud_tile(),
       "reps": a.reps, "inner": a.inner, "hbm_bytes_per_s": HBM_BYTES_PER_S, "rows": [], "baseline": {}, "rig": {}}
for B in [int(b) for b in a.batches.split(",")]:
    sel = torch.arange(B) % d1_all.shape[0]
    d1, colors = d1_all[sel].contiguous(), col_all[sel].contiguous()
    for crop in (False, True):
        for step in (1, 4):
            for dtype in ("f32", "f64"):
                for with_colors in (True, False):
                    fn, count_only, xyz, color, counts, cap = fused_call(d1, colors if with_colors else None, crop, step, dtype)
                    med, best, worst = time_events(fn, a.reps, a.inner)
                    count_med = time_events(count_only, a.reps, a.inner)[0]
                    kept = float(counts.sum().item())
                    nbytes = B * cap * 4 * 2 + kept * ((4 if with_colors else 0) + (12 if dtype == "f32" else 24) + (4 if with_colors else 0))
                    row = {"batch": B, "crop": "cli" if crop else "none", "step": step, "dtype": dtype, "colors": with_colors, "us_per_pair": med / B,
                           "count_and_scan_us_per_pair": count_med / B,
                           "us_per_pair_min_max": [best / B, worst / B], "kept_share_of_visited": kept / (B * cap), "kept_per_pair": kept / B,
                           "bytes_per_pair": nbytes / B, "bytes_per_s": nbytes / (med * 1e-6), "fraction_of_hbm": nbytes / (med * 1e-6) / HBM_BYTES_PER_S}
                    res["rows"].append(row)
                    print("B=%-3d crop %-4s step %d %s colours %-5s %9.3f us/pair [%8.3f %8.3f]  count+scan %8.3f  kept %.3f  %7.1f GB/s (%.3f of HBM)" % (
                        B, row["crop"], step, dtype, with_colors, row["us_per_pair"], best / B, worst / B, count_med / B, row["kept_share_of_visited"], row["bytes_per_s"] / 1e9,
                        row["fraction_of_hbm"]), flush=True)
                    del xyz, color, counts

# (b) before the fused call: the dense cloud written, then torch's mask, crop, boolean indexing, .float() and colour gather
B = 256
sel = torch.arange(B) % d1_all.shape[0]
d1, colors = d1_all[sel].contiguous(), col_all[sel].contiguous()
lo_t, hi_t = [float(v) for v in CLI_LO], [float(v) for v in CLI_HI]


def fused():
    return eng.compact_cloud_from_disparity(d1, Q, colors=colors, XR=XR, lo=CLI_LO, hi=CLI_HI, disparity="dmap", dtype="f32")


def unfused():
    dmap, cloud = eng.reproject(d1, Q, XR, None)
    m = dmap > 0
    for k in range(3):
        m = m & (cloud[..., k] > lo_t[k]) & (cloud[..., k] < hi_t[k])
    return cloud[m].float(), colors[m], m.reshape(B, -1).sum(1, dtype=torch.int32)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


f_xyz, f_col, _, f_counts = fused()
u_xyz, u_col, u_counts = unfused()
assert torch.equal(f_counts, u_counts), "the fused and the unfused counts differ"
parts = eng.split_clouds(f_xyz, f_counts, f_col)
assert torch.equal(torch.cat([p for p, _ in parts]).view(torch.int32), u_xyz.view(torch.int32)), "the fused and the unfused points differ"
assert torch.equal(torch.cat([c for _, c in parts]), u_col), "the fused and the unfused colours differ"
kept_b = int(f_counts.sum().item())
del f_xyz, f_col, u_xyz, u_col, parts
torch.cuda.empty_cache()
wall(fused), wall(unfused)
t_f, t_u = [], []
for _ in range(a.e2e_reps):
    t_f.append(wall(fused)[0])
    t_u.append(wall(unfused)[0])
res["baseline"] = {"batch": B, "disparity": "dmap", "dtype": "f32", "colors": True, "crop": "cli", "identical_results": True, "kept_points": kept_b,
                   "fused_ms": float(np.median(t_f)) * 1e3, "fused_ms_min_max": [min(t_f) * 1e3, max(t_f) * 1e3],
                   "reproject_plus_torch_ms": float(np.median(t_u)) * 1e3, "reproject_plus_torch_ms_min_max": [min(t_u) * 1e3, max(t_u) * 1e3],
                   "unfused_over_fused": float(np.median(t_u) / np.median(t_f)), "cloud_bytes": B * H * W * 24,
                   "fused_is_faster": bool(np.median(t_f) < np.median(t_u))}
print("B=256, CLI crop, dmap, f32, colours: fused %.3f ms, reproject + torch mask and gather %.1f ms: %.1fx" % (
    res["baseline"]["fused_ms"], res["baseline"]["reproject_plus_torch_ms"], res["baseline"]["unfused_over_fused"]), flush=True)
torch.cuda.empty_cache()

# (c) rig.compact_clouds vs rig.disparity, B = 64, device-resident BGR frames, alternated
B = 64
lb = torch.from_numpy(np.ascontiguousarray(np.stack([ls[k % 5] for k in range(B)])[..., ::-1])).cuda()
rb = torch.from_numpy(np.ascontiguousarray(np.stack([rs[k % 5] for k in range(B)])[..., ::-1])).cuda()
kw = dict(lo=CLI_LO, hi=CLI_HI, transform=(XR, None))
rig.disparity(lb, rb, pixel_format="bgr")
rig.compact_clouds(lb, rb, **kw)
t_d, t_c = [], []
for _ in range(a.e2e_reps):
    t_d.append(wall(lambda: rig.disparity(lb, rb, pixel_format="bgr"))[0])
    t_c.append(wall(lambda: rig.compact_clouds(lb, rb, **kw))[0])
e2e = {"batch": B, "disparity_pairs_per_s": B / float(np.median(t_d)), "compact_clouds_pairs_per_s": B / float(np.median(t_c))}
e2e["ratio"] = e2e["compact_clouds_pairs_per_s"] / e2e["disparity_pairs_per_s"]
res["rig"] = e2e
print("rig, batch %d: compact_clouds %.0f pairs/s, disparity %.0f pairs/s, ratio %.3f" % (B, e2e["compact_clouds_pairs_per_s"], e2e["disparity_pairs_per_s"],
                                                                                          e2e["ratio"]))
rig.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
if a.history:
    def row_of(batch, crop, step, dtype, colours):
        return next(r for r in res["rows"] if (r["batch"], r["crop"], r["step"], r["dtype"], r["colors"]) == (batch, crop, step, dtype, colours))

    big = max(int(b) for b in a.batches.split(","))
    r0, r1, r2 = row_of(big, "cli", 1, "f32", True), row_of(big, "none", 1, "f64", True), row_of(big, "cli", 4, "f32", True)
    b = res["baseline"]
    with open(a.history, "a") as f:
        f.write("\n## Compact coloured point clouds (`tools/compact_cloud_time.py`, `profiles/compact_cloud_time.json`)\n\n")
        f.write("* Fused disparity -> compact cloud (count, scan, write; KITTI %d x %d, d1, vehicle axes) at B = %d: CLI crop, f32, colours %.2f us per pair "
                "(kept share %.3f, %.0f GB/s of its own bytes = %.3f of 8 TB/s); no crop, f64, colours %.2f us (kept %.3f, %.3f of 8 TB/s); CLI crop, "
                "step 4 %.2f us.\n" % (W, H, big, r0["us_per_pair"], r0["kept_share_of_visited"], r0["bytes_per_s"] / 1e9, r0["fraction_of_hbm"],
                                      r1["us_per_pair"], r1["kept_share_of_visited"], r1["fraction_of_hbm"], r2["us_per_pair"]))
        f.write("* Against reproject() + torch mask, crop, boolean indexing, .float() and colour gather at B = %d (identical results asserted): %.2f ms "
                "fused, %.1f ms unfused, %.1fx.\n" % (b["batch"], b["fused_ms"], b["reproject_plus_torch_ms"], b["unfused_over_fused"]))
        f.write("* `rig.compact_clouds` %.0f pairs/s against `rig.disparity` %.0f pairs/s at B = %d (ratio %.3f).\n" % (
            e2e["compact_clouds_pairs_per_s"], e2e["disparity_pairs_per_s"], e2e["batch"], e2e["ratio"]))
