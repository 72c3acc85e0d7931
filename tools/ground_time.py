#!/usr/bin/env python3
"""Ground plane, obstacle labels and free space on KITTI maps resident in HBM (HIP events, median of --reps samples, each sample --inner
calls back to back; min / max beside the median):
  (a) ms per call of sv_ground_disparity_device at B = 1, 16, 256 on the engine's float disparity (disp_max 255: 1024 bins), default
      spec (steps 2, tol 2): the whole call, and its kernels by difference of calls that leave work out -
        histogram + prefix sums   a call with one candidate (vh_lo = vh_hi, qb_step = n_bins - 1) and no labels / free space
        search + pick             the call without labels / free space, minus the line above
        labels + free space       the whole call minus the call without labels / free space;
  (b) the histogram kernel with and without wavefront aggregation (SV_GROUND_HIST=plain), alternated, same outputs asserted;
  (c) the same result computed unfused with torch ops on the device - one bincount over (row, bin) indices for the histogram, cumsum
      and gathers per horizon row for the search, elementwise labels, a windowed sum for the free space -, identical results
      asserted before timing, alternated with the fused call, wall clock around a device synchronise.
The maps are the engine's d1 of the committed KITTI frames (tests/golden), repeated to fill the batch.

    python tools/ground_time.py [--reps 20] [--inner 5] [--batches 1,16,256]
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
ap.add_argument("--e2e-reps", type=int, default=5)
ap.add_argument("--batches", default="1,16,256")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
L = eng.ground_lib()
W, H, DISP_MAX = 1242, 375, 255
G = os.path.join(ROOT, "tests", "golden")


def png(name):
    return np.asarray(Image.open(os.path.join(G, name)))


def gray3(name):
    return np.ascontiguousarray(np.repeat(png(name)[..., None], 3, -1))


ls = [png("kitti0_color_left.png")] + [gray3("kitti%d_left.png" % k) for k in (1, 2, 3, 4)]
rs = [png("kitti0_color_right.png")] + [gray3("kitti%d_right.png" % k) for k in (1, 2, 3, 4)]
rig = rigmod.StereoRig(W, H)
d1_all = rig.disparity(torch.from_numpy(np.stack(ls)).cuda(), torch.from_numpy(np.stack(rs)).cuda(), pixel_format="rgb")
rig.close()


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


def fused_call(d1, spec, vdisp=True, rest=True):
    """A closure that enqueues the C entry on pre-allocated outputs and workspace (no allocation in the timed window), and its outputs."""
    B = d1.shape[0]
    out = {"ground": torch.empty((B, 4), dtype=torch.int32, device="cuda")}
    if vdisp:
        out["vdisp"] = torch.empty((B, H, spec.n_bins), dtype=torch.int32, device="cuda")
    if rest:
        out["labels"] = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
        out["free_row"] = torch.empty((B, W), dtype=torch.int32, device="cuda")
        out["free_disp"] = torch.empty((B, W), dtype=torch.float32, device="cuda")
    nbytes = L.sv_ground_workspace_bytes(ctypes.byref(spec), B, W, H)
    ws = torch.empty((nbytes // 8 + 1,), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda k: out[k].data_ptr() if k in out else None  # noqa: E731

    def fn():
        rc = L.sv_ground_disparity_device(d1.data_ptr(), B, W, H, ctypes.byref(spec), ptr("vdisp"), ptr("ground"), ptr("labels"), ptr("free_row"), ptr("free_disp"),
                                          ws.data_ptr(), nbytes, st)
        assert rc == 0

    return fn, out


spec = eng.ground_spec(H, DISP_MAX, min_support=W)
one = eng.ground_spec(H, DISP_MAX, vh_lo=168, vh_hi=168, qb_step=spec.n_bins - 1, min_support=W)
n_vh, n_qb = (spec.vh_hi - spec.vh_lo) // spec.vh_step + 1, (spec.n_bins - 1) // spec.qb_step
lookups = sum((H - max(vh + 1, 0)) * n_qb for vh in range(spec.vh_lo, spec.vh_hi + 1, spec.vh_step))
print("KITTI %d x %d, %d bins, %d x %d candidates, %.2f M box lookups per pair; reps %d, inner %d" % (W, H, spec.n_bins, n_vh, n_qb, lookups / 1e6, a.reps, a.inner))
print("(a) ms per call [min max]: whole call | histogram + prefix | search + pick (difference) | labels + free space (difference)")
for B in [int(b) for b in a.batches.split(",")]:
    d1 = d1_all[torch.arange(B) % d1_all.shape[0]].contiguous()
    whole, _ = fused_call(d1, spec)
    line, _ = fused_call(d1, spec, vdisp=False, rest=False)
    hist, _ = fused_call(d1, one, vdisp=False, rest=False)
    tw, tl, th = time_events(whole, a.reps, a.inner), time_events(line, a.reps, a.inner), time_events(hist, a.reps, a.inner)
    print("B=%-3d whole %8.4f [%8.4f %8.4f] | hist %8.4f [%8.4f %8.4f] | search %8.4f | labels %8.4f | %.2f us per pair, %.1f G lookups/s" % (
        B, tw[0], tw[1], tw[2], th[0], th[1], th[2], tl[0] - th[0], tw[0] - tl[0], tw[0] * 1e3 / B, lookups * B / ((tl[0] - th[0]) * 1e-3) / 1e9), flush=True)

# (b) the histogram kernel with and without wavefront aggregation
B = max(int(b) for b in a.batches.split(","))
d1 = d1_all[torch.arange(B) % d1_all.shape[0]].contiguous()
hist, out = fused_call(d1, one, vdisp=True, rest=False)
os.environ.pop("SV_GROUND_HIST", None)
hist()
torch.cuda.synchronize()
agg_vdisp = out["vdisp"].clone()
os.environ["SV_GROUND_HIST"] = "plain"
hist()
torch.cuda.synchronize()
assert torch.equal(agg_vdisp, out["vdisp"]), "the two histogram kernels differ"
t_agg, t_plain = [], []
for _ in range(3):
    os.environ.pop("SV_GROUND_HIST", None)
    t_agg.append(time_events(hist, a.reps, a.inner)[0])
    os.environ["SV_GROUND_HIST"] = "plain"
    t_plain.append(time_events(hist, a.reps, a.inner)[0])
os.environ.pop("SV_GROUND_HIST", None)
nb = B * H * (W * 4 + spec.n_bins * 4 + (spec.n_bins + 1) * 4)
print("(b) B=%d histogram + prefix sums (vdisp stored): aggregated per wavefront %s ms, one atomic per pixel %s ms; same counts; %.0f GB/s of its own "
      "bytes aggregated" % (B, ["%.4f" % t for t in t_agg], ["%.4f" % t for t in t_plain], nb / (float(np.median(t_agg)) * 1e-3) / 1e9), flush=True)

# (c) the same result with torch ops
whole, out = fused_call(d1, spec)
whole()
torch.cuda.synchronize()


def unfused():
    nbn = spec.n_bins
    valid = d1 > 0
    q = torch.where(valid, torch.clamp(torch.round(d1 * 4.0), max=float(nbn - 1)), torch.zeros_like(d1)).long()
    rowbin = (torch.arange(B * H, device="cuda").view(B, H, 1) * nbn + q)[valid]
    vdisp = torch.bincount(rowbin, minlength=B * H * nbn).view(B, H, nbn)
    P = torch.zeros((B, H, nbn + 1), dtype=torch.int64, device="cuda")
    P[:, :, 1:] = vdisp.cumsum(2)
    qbs = torch.arange(spec.qb_step, nbn, spec.qb_step, device="cuda")
    best_S = torch.full((B,), -1, dtype=torch.int64, device="cuda")
    best_vh, best_qb = torch.zeros_like(best_S), torch.zeros_like(best_S)
    for vh in range(spec.vh_lo, spec.vh_hi + 1, spec.vh_step):
        den = H - 1 - vh
        v = torch.arange(max(vh + 1, 0), H, device="cuda")
        ql = (2 * qbs[None, :] * (v[:, None] - vh) + den) // (2 * den)
        rows = P[:, v]
        hi = torch.clamp(ql + spec.tol + 1, max=nbn).unsqueeze(0).expand(B, -1, -1)
        lo = torch.clamp(ql - spec.tol, min=0).unsqueeze(0).expand(B, -1, -1)
        S = (rows.gather(2, hi) - rows.gather(2, lo)).sum(1)
        s, i = S.max(1)
        i = (S == s[:, None]).int().argmax(1)  # the first of equal maxima
        better = s > best_S
        best_S, best_vh, best_qb = torch.where(better, s, best_S), torch.where(better, torch.full_like(s, vh), best_vh), torch.where(better, qbs[i], best_qb)
    found = best_S >= spec.min_support
    vv = torch.arange(H, device="cuda")[None, :]
    den = (H - 1 - best_vh)[:, None]
    g = torch.where(vv > best_vh[:, None], (2 * best_qb[:, None] * (vv - best_vh[:, None]) + den) // (2 * den), torch.zeros_like(vv))
    e = q - g[:, :, None]
    labels = torch.where(e > spec.g_tol, 2, torch.where(e < -spec.g_tol, 3, 1))
    labels = torch.where(valid, torch.where(found[:, None, None], labels, torch.full_like(labels, 3)), torch.zeros_like(labels)).to(torch.uint8)
    ob = (labels == 2).flip(1).long()  # row 0 = the bottom row
    cs = torch.zeros((B, H + 1, W), dtype=torch.int64, device="cuda")
    cs[:, 1:] = ob.cumsum(1)
    full = (cs[:, spec.min_run:] - cs[:, :H + 1 - spec.min_run]) == spec.min_run  # [B, H + 1 - min_run, W]: a run starts at flipped row k
    any_run = full.any(1)
    k = full.int().argmax(1)
    free_row = torch.where(any_run, H - 1 - k, torch.full_like(k, -1)).int()
    free_disp = torch.where(any_run, d1.gather(1, (H - 1 - k).clamp(min=0).unsqueeze(1)).squeeze(1), torch.zeros((B, W), device="cuda"))
    ground = torch.stack([torch.where(found, best_vh, torch.full_like(best_vh, -1)), torch.where(found, best_qb, torch.full_like(best_qb, -1)), best_S, valid.sum((1, 2))], 1).int()
    return {"vdisp": vdisp.int(), "ground": ground, "labels": labels, "free_row": free_row, "free_disp": free_disp}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


ref = unfused()
for k in out:
    assert torch.equal(out[k], ref[k]), "the fused and the unfused %s differ" % k
del ref
torch.cuda.empty_cache()
wall(whole), wall(unfused)
t_f, t_u = [], []
for _ in range(a.e2e_reps):
    t_f.append(wall(whole)[0])
    t_u.append(wall(unfused)[0])
print("(c) B=%d, identical results: fused %.3f ms [%.3f %.3f], torch bincount / cumsum / gathers %.1f ms [%.1f %.1f]: %.1fx" % (
    B, np.median(t_f) * 1e3, min(t_f) * 1e3, max(t_f) * 1e3, np.median(t_u) * 1e3, min(t_u) * 1e3, max(t_u) * 1e3, np.median(t_u) / np.median(t_f)))
