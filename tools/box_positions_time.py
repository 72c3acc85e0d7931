#!/usr/bin/env python3
"""Object positions per detector box on KITTI maps (HIP events, median of --reps samples, each sample --inner calls back to back):
  (a) us per pair of the fused disparity -> positions call (one kernel), select "near" / "valid" / "all" on the float disparity ("d1"),
      at B = 1, 16, 256 with 16 seeded boxes per pair (40-300 pixels wide, 40-200 high) and with ONE full-frame box per pair (a thread
      owns a column, so that box is 1241 columns as five sequential chunks of 374 rows in one workgroup: the layout's weak spot);
  (b) the comparison with what the batch API offered before the fused call, for the same 16 boxes per pair at B = 256: reproject() to
      an f64 cloud plus one torch slice-and-sum per box, alternated with the fused "all" / "dmap" call (the same quantity) in this
      process, wall clock around a device synchronise;
  (c) rig.box_positions against rig.disparity, pairs/s at B = 64 on device-resident BGR frames, alternated.
The maps are the engine's d1 of the committed KITTI frames (tests/golden), repeated to fill the batch.

    python tools/box_positions_time.py [--reps 20] [--inner 5] [--out profiles/box_positions_time.json]
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
L = eng.box_lib()
W, H, M = 1242, 375, 16
G = os.path.join(ROOT, "tests", "golden")


def png(name):
    return np.asarray(Image.open(os.path.join(G, name)))


def gray3(name):
    return np.ascontiguousarray(np.repeat(png(name)[..., None], 3, -1))


ls = [png("kitti0_color_left.png")] + [gray3("kitti%d_left.png" % k) for k in (1, 2, 3, 4)]
rs = [png("kitti0_color_right.png")] + [gray3("kitti%d_right.png" % k) for k in (1, 2, 3, 4)]
rig = rigmod.StereoRig(W, H)
d1_all = rig.disparity(torch.from_numpy(np.stack(ls)).cuda(), torch.from_numpy(np.stack(rs)).cuda(), pixel_format="rgb")
Q = rig.Q.copy()
q = np.ascontiguousarray(Q, np.float64).reshape(16)


def seeded_boxes(B, seed=1):
    rng = np.random.default_rng(seed)
    bw, bh = rng.integers(40, 301, (B, M)), rng.integers(40, 201, (B, M))
    x, y = (rng.random((B, M)) * (W - 1 - bw)).astype(np.int64), (rng.random((B, M)) * (H - 1 - bh)).astype(np.int64)  # inside the map
    return np.stack([x, y, bw, bh], -1).astype(np.int32)


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


def fused_call(d1, boxes, select, disparity, band=4):
    """A closure that enqueues the C entry on pre-allocated outputs (no allocation in the timed window)."""
    B, m = boxes.shape[:2]
    spec = eng.box_spec(select, disparity, band)
    pos = torch.empty((B, m, 3), dtype=torch.float64, device="cuda")
    stat = torch.empty((B, m, 4), dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def fn():
        rc = L.sv_box_positions_disparity_device(d1.data_ptr(), B, W, H, q.ctypes.data, None, None, boxes.data_ptr(), None, m, ctypes.byref(spec),
                                                 pos.data_ptr(), stat.data_ptr(), st)
        assert rc == 0

    return fn, pos, stat


res = {"width": W, "height": H, "boxes_per_pair": M, "disparity": "d1", "band": 4, "reps": a.reps, "inner": a.inner, "rows": [], "baseline": {}, "rig": {}}
for B in [int(b) for b in a.batches.split(",")]:
    d1 = d1_all[torch.arange(B) % d1_all.shape[0]].contiguous()
    shapes = {"16 boxes": torch.from_numpy(seeded_boxes(B)).cuda(),
              "full frame": torch.tensor([0, 0, W, H], dtype=torch.int32, device="cuda").repeat(B, 1, 1)}
    for shape, boxes in shapes.items():
        row = {"batch": B, "boxes": shape, "pixels_per_pair": None}
        for select in ("near", "valid", "all"):
            fn, pos, stat = fused_call(d1, boxes, select, "d1")
            med, best, worst = time_events(fn, a.reps, a.inner)
            row[select + "_us_per_pair"] = med / B
            row[select + "_us_per_pair_min_max"] = [best / B, worst / B]
            row["pixels_per_pair"] = float(stat[..., 0].sum().item()) / B
            row[select + "_selected_share"] = float(stat[..., 3].sum().item()) / max(float(stat[..., 0].sum().item()), 1.0)
        res["rows"].append(row)
        print("B=%-3d %-10s %8.0f pixels/pair  near %8.3f  valid %8.3f  all %8.3f us/pair" % (B, shape, row["pixels_per_pair"], row["near_us_per_pair"],
                                                                                            row["valid_us_per_pair"], row["all_us_per_pair"]), flush=True)

# (b) before the fused call: the cloud written, then one slice-and-sum per box, against the fused "all" / "dmap" call
B = 256
d1 = d1_all[torch.arange(B) % d1_all.shape[0]].contiguous()
boxes_np = seeded_boxes(B)
boxes = torch.from_numpy(boxes_np).cuda()
fused, pos, _ = fused_call(d1, boxes, "all", "dmap")


def unfused():
    _, cloud = eng.reproject(d1, Q, want_dmap=False)
    out = torch.empty((B, M, 3), dtype=torch.float64, device="cuda")
    for b in range(B):
        for m in range(M):
            x, y, w, h = boxes_np[b, m]
            out[b, m] = cloud[b, y:y + h, x:x + w].sum(dim=(0, 1)) / float(w * h)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


wall(fused), wall(unfused)
t_f, t_u = [], []
for _ in range(a.e2e_reps):
    t, _ = wall(fused)
    t_f.append(t)
    t, ref = wall(unfused)
    t_u.append(t)
both = torch.isfinite(ref) & torch.isfinite(pos)
res["baseline"] = {"batch": B, "fused_ms": float(np.median(t_f)) * 1e3, "fused_ms_min_max": [min(t_f) * 1e3, max(t_f) * 1e3],
                   "reproject_plus_torch_slices_ms": float(np.median(t_u)) * 1e3, "reproject_plus_torch_slices_ms_min_max": [min(t_u) * 1e3, max(t_u) * 1e3],
                   "speedup": float(np.median(t_u) / np.median(t_f)), "cloud_bytes": B * H * W * 24,
                   "same_non_finite_pattern": bool((torch.isfinite(ref) == torch.isfinite(pos)).all().item()),
                   "finite_results": int(both.sum().item()),
                   "max_relative_difference_where_finite": float(((ref - pos).abs() / ref.abs().clamp_min(1e-300))[both].max().item()) if both.any() else 0.0}
print("B=256, 16 boxes/pair, all/dmap: fused %.3f ms, reproject + %d torch slices %.1f ms: %.0fx" % (res["baseline"]["fused_ms"], B * M,
      res["baseline"]["reproject_plus_torch_slices_ms"], res["baseline"]["speedup"]), flush=True)
del ref, pos
torch.cuda.empty_cache()

# (c) rig.box_positions vs rig.disparity, B = 64, device-resident BGR frames, alternated
B = 64
lb = torch.from_numpy(np.ascontiguousarray(np.stack([ls[k % 5] for k in range(B)])[..., ::-1])).cuda()
rb = torch.from_numpy(np.ascontiguousarray(np.stack([rs[k % 5] for k in range(B)])[..., ::-1])).cuda()
bx = torch.from_numpy(seeded_boxes(B)).cuda()
rig.disparity(lb, rb, pixel_format="bgr")
rig.box_positions(lb, rb, bx)
t_d, t_b = [], []
for _ in range(a.e2e_reps):
    t, _ = wall(lambda: rig.disparity(lb, rb, pixel_format="bgr"))
    t_d.append(t)
    t, _ = wall(lambda: rig.box_positions(lb, rb, bx))
    t_b.append(t)
e2e = {"batch": B, "disparity_pairs_per_s": B / float(np.median(t_d)), "box_positions_pairs_per_s": B / float(np.median(t_b))}
e2e["ratio"] = e2e["box_positions_pairs_per_s"] / e2e["disparity_pairs_per_s"]
res["rig"] = e2e
print("rig, batch %d: box_positions %.0f pairs/s, disparity %.0f pairs/s, ratio %.3f" % (B, e2e["box_positions_pairs_per_s"], e2e["disparity_pairs_per_s"], e2e["ratio"]))
rig.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
