#!/usr/bin/env python3
"""Stixels and detector-free object boxes on KITTI maps resident in HBM (HIP events, median of --reps samples, each sample --inner
calls back to back; min / max beside the median):
  (a) ms per call of sv_stixel_disparity_device at B = 1, 16, 256 on the engine's float disparity (disp_max 255: 1024 bins) and the
      labels of sv_ground_disparity_device, default spec: the whole call, the column kernel alone (SV_STIXEL_STAGE=columns) and the
      object kernel by difference; the call's own bytes (4 N of disparity, N of labels, the stixel rows written) over its time
      against the 6.29 TB/s copy ceiling; beside it, in the same run, the label kernel of sv_ground_disparity_device on the same maps
      (the whole ground call minus the call without labels / free space) and the ratio of the two walks;
  (b) rig.objects against rig.ground, B = 64, alternated, wall clock around a device synchronise.
The maps are the engine's d1 of the committed KITTI frames (tests/golden), repeated to fill the batch.

    python tools/stixel_time.py [--reps 20] [--inner 5] [--batches 1,16,256]
"""
import argparse
import ctypes
import importlib
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
ap.add_argument("--e2e-reps", type=int, default=7)
ap.add_argument("--batches", default="1,16,256")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
L, LG = eng.stixel_lib(), eng.ground_lib()
W, H, DISP_MAX, COPY_CEILING = 1242, 375, 255, 6.29e12
G = os.path.join(ROOT, "tests", "golden")


def png(name):
    return np.asarray(Image.open(os.path.join(G, name)))


def gray3(name):
    return np.ascontiguousarray(np.repeat(png(name)[..., None], 3, -1))


ls = np.stack([png("kitti0_color_left.png")] + [gray3("kitti%d_left.png" % k) for k in (1, 2, 3, 4)])
rs = np.stack([png("kitti0_color_right.png")] + [gray3("kitti%d_right.png" % k) for k in (1, 2, 3, 4)])
rig = rigmod.StereoRig(W, H)
d1_all = rig.disparity(torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda(), pixel_format="rgb")


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
        ts.append(e0.elapsed_time(e1) / inner)  # ms per call
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def stixel_call(d1, labels, spec, capacity=64):
    """A closure that enqueues the C entry on pre-allocated outputs and workspace (no allocation in the timed window), and its outputs."""
    B = d1.shape[0]
    out = {"stixels": torch.empty((B, spec.max_layers, W, 4), dtype=torch.int32, device="cuda"), "n_stixels": torch.empty((B, W), dtype=torch.int32, device="cuda"),
           "boxes": torch.zeros((B, capacity, 4), dtype=torch.int32, device="cuda"), "info": torch.zeros((B, capacity, 4), dtype=torch.int32, device="cuda"),
           "counts": torch.zeros((B,), dtype=torch.int32, device="cuda")}
    nbytes = L.sv_stixel_workspace_bytes(ctypes.byref(spec), B, W, H)
    ws = torch.empty((nbytes // 8 + 1,), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def fn():
        rc = L.sv_stixel_disparity_device(d1.data_ptr(), labels.data_ptr(), B, W, H, ctypes.byref(spec), capacity, out["stixels"].data_ptr(), out["n_stixels"].data_ptr(),
                                          out["boxes"].data_ptr(), out["info"].data_ptr(), out["counts"].data_ptr(), ws.data_ptr(), nbytes, st)
        assert rc == 0

    return fn, out


def ground_call(d1, spec, rest):
    B = d1.shape[0]
    ground = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    labels = torch.empty((B, H, W), dtype=torch.uint8, device="cuda") if rest else None
    free_row = torch.empty((B, W), dtype=torch.int32, device="cuda") if rest else None
    free_disp = torch.empty((B, W), dtype=torch.float32, device="cuda") if rest else None
    nbytes = LG.sv_ground_workspace_bytes(ctypes.byref(spec), B, W, H)
    ws = torch.empty((nbytes // 8 + 1,), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def fn():
        rc = LG.sv_ground_disparity_device(d1.data_ptr(), B, W, H, ctypes.byref(spec), None, ground.data_ptr(), ptr(labels), ptr(free_row), ptr(free_disp), ws.data_ptr(),
                                           nbytes, st)
        assert rc == 0

    return fn


spec = eng.stixel_spec(DISP_MAX)
gspec = eng.ground_spec(H, DISP_MAX, min_support=W)
print("KITTI %d x %d, %d bins, q_min %d sim %d max_gap %d min_rows %d max_layers %d col_step %d sim_cols %d min_cols %d; reps %d, inner %d" % (
    W, H, spec.n_bins, spec.q_min, spec.sim, spec.max_gap, spec.min_rows, spec.max_layers, spec.col_step, spec.sim_cols, spec.min_cols, a.reps, a.inner))
print("(a) ms per call [min max]: whole call | column kernel alone | object kernel (difference) | ground's label kernel (difference), same maps")
for B in [int(b) for b in a.batches.split(",")]:
    d1 = d1_all[torch.arange(B) % d1_all.shape[0]].contiguous()
    labels = eng.ground_from_disparity(d1, DISP_MAX, want_vdisp=False, want_free=False).labels
    whole, out = stixel_call(d1, labels, spec)
    os.environ.pop("SV_STIXEL_STAGE", None)
    tw = time_events(whole, a.reps, a.inner)
    os.environ["SV_STIXEL_STAGE"] = "columns"
    tc = time_events(whole, a.reps, a.inner)
    os.environ.pop("SV_STIXEL_STAGE", None)
    whole()
    torch.cuda.synchronize()
    tg_all, tg_line = time_events(ground_call(d1, gspec, True), a.reps, a.inner), time_events(ground_call(d1, gspec, False), a.reps, a.inner)
    t_label = tg_all[0] - tg_line[0]
    n_st = torch.clamp(out["n_stixels"], max=spec.max_layers).sum().item()
    # read: 4 N of disparity and N of labels; written: every stored stixel row and its -1 fill (16 bytes each), n_stixels and the first layer
    nb = B * H * W * 5 + B * W * (16 * spec.max_layers + 4 + 16)
    print("B=%-3d whole %8.4f [%8.4f %8.4f] | columns %8.4f [%8.4f %8.4f] | objects %8.4f | ground labels %8.4f | %.2f us per pair whole, %.2f us columns; "
          "columns / ground labels %.2f; %.0f GB/s of its own bytes in the column kernel = %.3f of the copy ceiling; %.1f objects and %.0f stored stixels per pair" % (
              B, tw[0], tw[1], tw[2], tc[0], tc[1], tc[2], tw[0] - tc[0], t_label, tw[0] * 1e3 / B, tc[0] * 1e3 / B, tc[0] / t_label,
              nb / (tc[0] * 1e-3) / 1e9, nb / (tc[0] * 1e-3) / COPY_CEILING, out["counts"].float().mean().item(), n_st / B), flush=True)


# (b) the rig: objects against ground
def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


B = 64
tl = torch.from_numpy(ls).cuda()[torch.arange(B) % len(ls)].contiguous()
tr = torch.from_numpy(rs).cuda()[torch.arange(B) % len(rs)].contiguous()
f_obj = lambda: rig.objects(tl, tr, pixel_format="rgb")  # noqa: E731
f_gnd = lambda: rig.ground(tl, tr, pixel_format="rgb")  # noqa: E731
wall(f_obj), wall(f_gnd)
t_o, t_g = [], []
for _ in range(a.e2e_reps):
    t_o.append(wall(f_obj))
    t_g.append(wall(f_gnd))
print("(b) B=%d: rig.objects %.0f pairs/s [%.2f ms, %.2f .. %.2f], rig.ground %.0f pairs/s [%.2f ms, %.2f .. %.2f]: ratio %.3f" % (
    B, B / np.median(t_o), np.median(t_o) * 1e3, min(t_o) * 1e3, max(t_o) * 1e3, B / np.median(t_g), np.median(t_g) * 1e3, min(t_g) * 1e3, max(t_g) * 1e3,
    np.median(t_g) / np.median(t_o)))
rig.close()
