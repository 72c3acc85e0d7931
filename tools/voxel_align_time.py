#!/usr/bin/env python3
"""A frame aligned to the voxel map on a synthetic street (HIP events, median of --reps calls after warm-up, min / max beside the median;
one process).  The map, at --size metres, is tools/voxel_clusters_time.py's: a ground plane of 800 x 800 cells and on it a grid of 66 x 66
blocks of 3 x 3 x 9 cells, twelve cells apart - about a million voxels.  Two frames stand in it, both within 20 m of the vehicle and
started off their true pose by 0.45 degrees (roll, pitch and yaw; 0.8 cells at 20 m) and 0.7 cells - what a coarse search leaves:
  voxel rows    one row per voxel the vehicle sees, at the voxel's centre plus noise - what voxel_cloud gives;
  compact cloud --cloud-rows rows (300 000 by default) on the same surfaces, many per voxel - what compact_cloud gives.
Per frame:
  (a) us per call of sv_voxel_align_device (one round: the sums only) into pre-allocated outputs and workspace, without and with the
      per-row outputs;
  (b) the table look-ups the definition asks for - a kept row's cells inside the box, at most 27 - per microsecond of that call;
  (c) the choices of the kernels, each beside the default in the same run and alternating with it: every one of the 27 cells looked into
      instead of leaving out those whose bound exceeds the best so far (sv_debug_voxel_align's flag), and at most 128 and 32 chunks of
      rows per frame instead of 512;
  (d) a whole engine.voxel_map_align of 10 rounds (eps 0, so none is spared), by the host's clock: it ends in the read-back of a round;
  (e) the unfused form on the same device with torch ops - the map's voxels as sorted keys and positions (made once, outside the timed
      part), then per round the transform, the cells, 27 searchsorted look-ups with their gathers, the nearest by where(), and the sums -
      for one round and for the 10 rounds with the same host fit.  Before anything is timed both forms must agree on all 19 sums.
The yardstick is never the code under test.  Nothing is asserted about speed: fused_is_faster is reported.

    timeout -k 10 900 python tools/voxel_align_time.py [--reps 21] [--out profiles/voxel_align_time.json]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "low-cost-hardware-accelerated-vision-based-depth-perception-for-real-time-applications_amd"
OFFSETS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def street_cells(side):
    """tools/voxel_clusters_time.py's street: int64 [V,3] cells, shuffled."""
    g = np.arange(side)
    ground = np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3)
    starts = np.arange(4, side - 4, 12)
    block = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(1, 10), indexing="ij"), -1).reshape(-1, 3)
    blocks = (np.stack(np.meshgrid(starts, starts, [0], indexing="ij"), -1).reshape(-1, 1, 3) + block).reshape(-1, 3)
    cells = np.concatenate([ground, blocks])
    return cells[np.random.default_rng(3).permutation(len(cells))]


def frames_of(cells, size, side, reach_m, cloud_rows, truth):
    """{"voxel_rows": xyz, "compact_cloud": xyz}: float32 [1,N,3] in the vehicle's axes at the pose `truth` (12 words)."""
    rng = np.random.default_rng(11)
    centre = truth[9:] / size
    seen = cells[(np.abs(cells[:, :2] + 0.5 - centre[:2]) < reach_m / size).all(1)]
    R, t = truth[:9].reshape(3, 3), truth[9:]
    world = {"voxel_rows": (seen + 0.5 + rng.uniform(-0.2, 0.2, seen.shape)) * size,
             "compact_cloud": (seen[rng.integers(0, len(seen), cloud_rows)] + rng.uniform(0.05, 0.95, (cloud_rows, 3))) * size}
    return {k: ((w - t) @ R).astype(np.float32)[None] for k, w in world.items()}  # Pf = R^T (Pw - t)


def index_of_table(table):
    """(vkey, vq): the table's voxels with n, m >= 1 as ascending keys and their positions in 1/256 of a cell."""
    key, n = table[:, 0], table[:, 1]
    live = ((key != -1) & (n >= 1) & (table[:, 9] >= 1) & ((table[:, 10] >> 32) >= 0)).nonzero(as_tuple=True)[0]
    e = table[live]
    vkey, by = torch.sort(e[:, 0])
    e = e[by]
    cell = torch.stack([(vkey >> (20 * k)) & 0xFFFFF for k in range(3)], -1)
    return vkey, 256 * cell + (torch.div(e[:, 2:5], e[:, 1:2], rounding_mode="floor") >> 8)


def torch_round(params, vkey, vq, xyz, pose, origin, max_d2):
    """The 19 sums of one frame (xyz [N,3], every weight 1) with torch ops, and the look-ups the definition asks for."""
    dev = xyz.device
    f = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)  # noqa: E731  (tensors: torch divides by a Python number as a product with its reciprocal)
    lo, hi, size, cells = f(params["lo"]), f(params["hi"]), f(params["size"]), torch.tensor(params["cells"], dtype=torch.int64, device=dev)
    X = xyz.double()
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    Pw = torch.stack([((pose[3 * k] * x + pose[3 * k + 1] * y) + pose[3 * k + 2] * z) + pose[9 + k] for k in range(3)], -1)
    keep = ((lo < Pw) & (Pw < hi)).all(-1)
    t = torch.where(keep[:, None], (Pw - lo) / size, torch.zeros_like(Pw))
    c = torch.minimum(t.long(), cells - 1)
    u = torch.clamp(((t - c.double()) * f(65536.0)).long(), max=65535)
    p = 256 * c + (u >> 8)
    N, V = xyz.shape[0], vkey.numel()
    best_d2 = torch.full((N,), 2 ** 40, dtype=torch.int64, device=dev)
    best_key = torch.full((N,), -1, dtype=torch.int64, device=dev)
    best_q = torch.zeros((N, 3), dtype=torch.int64, device=dev)
    lookups = 0
    for d in OFFSETS:
        cc = c + torch.tensor(d, dtype=torch.int64, device=dev)
        on = keep & ((cc >= 0) & (cc < cells)).all(-1)
        key = torch.where(on, cc[:, 0] | (cc[:, 1] << 20) | (cc[:, 2] << 40), torch.full_like(best_key, -2))
        at = torch.searchsorted(vkey, key).clamp(max=V - 1)
        q = vq[at]
        d2 = ((p - q) ** 2).sum(1)
        take = on & (vkey[at] == key) & ((d2 < best_d2) | ((d2 == best_d2) & (key < best_key)))
        best_d2, best_key, best_q = torch.where(take, d2, best_d2), torch.where(take, key, best_key), torch.where(take[:, None], q, best_q)
        lookups = lookups + on.sum()
    pair = ((best_key >= 0) & (best_d2 <= max_d2)).long()
    dp, dq = (p - origin) * pair[:, None], (best_q - origin) * pair[:, None]
    head = torch.stack([keep.sum(), pair.sum(), pair.sum(), (pair * best_d2).sum()])
    return torch.cat([head, dp.sum(0), dq.sum(0), (dp[:, :, None] * dq[:, None, :]).sum(0).reshape(9)]), lookups


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


def time_beside(fns, reps):
    """The calls of `fns` (a dict) timed in turns, so that a drift of the machine meets all of them alike."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"us": float(np.median(v)), "min_max": [float(np.min(v)), float(np.max(v))]} for k, v in ts.items()}


def time_host(fn, reps):
    """A call that ends in a read-back, by the host's clock."""
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return {"us": float(np.median(ts)), "min_max": [float(np.min(ts)), float(np.max(ts))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--size", type=float, default=0.2)
    ap.add_argument("--side", type=int, default=800, help="cells of the ground plane per axis")
    ap.add_argument("--cloud-rows", type=int, default=300000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    rigmod = importlib.import_module(PKG + ".rig")
    eng = importlib.import_module(PKG + ".engine")
    sv = importlib.import_module(PKG + ".stereo_vision.sv")
    L, A = eng.voxel_map_lib(), eng.voxel_align_lib()
    size, side = a.size, a.side
    st = torch.cuda.current_stream().cuda_stream

    cells = street_cells(side)
    cap = 65536
    B = -(-len(cells) // cap)
    xyz = np.zeros((B * cap, 3), np.float32)
    xyz[:len(cells)] = (cells + 0.5) * size
    counts = np.full(B, cap, np.int32)
    counts[-1] = len(cells) - (B - 1) * cap
    m = rigmod.VoxelMap((0.0, 0.0, 0.0), (side * size, side * size, 16 * size), size, len(cells) + len(cells) // 8)
    m.update(torch.from_numpy(xyz.reshape(B, cap, 3)).cuda(), None, None, torch.from_numpy(counts).cuda(), np.tile(sv.voxel_map_pose(0.0, 0.0, 0.0), (B, 1)))
    assert m.stats()["claimed"] == len(cells) and not m.stats()["overflowed"]
    params, buf = m.params, m.buffer
    spec, nbytes = eng.voxel_map_spec(params), L.sv_voxel_map_bytes(params["capacity"])
    slots = int(L.sv_voxel_map_slots(params["capacity"]))
    table = buf[4:4 + 11 * slots].view(slots, 11)  # behind the head of 32 bytes: key, n, S[3], C[4], m, first_seq | last_seq << 32
    vkey, vq = index_of_table(table)
    assert vkey.numel() == len(cells)

    truth = sv.voxel_map_pose(0.5 * side * size + 0.07, 0.5 * side * size - 0.04, 0.3, 1.2)
    cr, sr, cp, sp, cy, sy = np.cos(0.003), np.sin(0.003), np.cos(-0.004), np.sin(-0.004), np.cos(0.006), np.sin(0.006)
    off = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]]) @ np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    start = np.concatenate([(off @ truth[:9].reshape(3, 3)).reshape(9), truth[9:] + np.array([0.5, -0.4, 0.3]) * size])[None]
    origin = sv.voxel_align_origin(params, start)
    max_d2 = sv.voxel_align_max_d2(1.0)
    res = {"size": size, "voxels_in_the_map": len(cells), "capacity": params["capacity"], "table_slots": slots, "map_bytes": nbytes, "max_dist_cells": 1.0, "reps": a.reps, "runs": []}

    for name, frame in frames_of(cells, size, side, 20.0, a.cloud_rows, truth).items():
        fx, fc = torch.from_numpy(frame).cuda(), torch.tensor([frame.shape[1]], dtype=torch.int32, device="cuda")
        rows = frame.shape[1]
        pose_t, origin_t = torch.from_numpy(start).cuda(), torch.from_numpy(origin).cuda()
        out = eng.voxel_map_align_sums(buf, params, fx, None, fc, pose_t, origin_t, want_rows=True)
        need = ctypes.c_size_t()
        assert A.sv_voxel_align_workspace(rows, 1, ctypes.byref(need)) == 0
        ws = torch.empty((need.value // 8,), dtype=torch.int64, device="cuda")

        def call(per_row=False):
            rc = A.sv_voxel_align_device(buf.data_ptr(), nbytes, ctypes.byref(spec), fx.data_ptr(), 0, None, fc.data_ptr(), pose_t.data_ptr(), origin_t.data_ptr(), 1, rows,
                                         max_d2, 1, 1, 0, out.sums.data_ptr(), out.pair_key.data_ptr() if per_row else None, out.pair_d2.data_ptr() if per_row else None,
                                         ws.data_ptr(), need.value, st)
            assert rc == 0, L.sv_last_error(None)

        def hooked(max_chunks, skip):
            def fn():
                eng.debug_voxel_align(max_chunks, skip)
                call()
            return fn

        def unfused(pose=pose_t[0], o=origin_t[0].long()):
            return torch_round(params, vkey, vq, fx[0], pose, o, max_d2)

        call()
        slow, lookups = unfused()
        fused = out.sums[0].clone()
        assert torch.equal(fused, slow), "the fused and the unfused form disagree on the sums of %s: %s / %s" % (name, fused.tolist(), slow.tolist())
        lookups = int(lookups)
        entry = {"run": name, "rows": rows, "inside": int(fused[0]), "pairs": int(fused[1]), "lookups": lookups}
        entry["call_us"] = time_events(call, a.reps)
        entry["call_per_row_us"] = time_events(lambda: call(True), a.reps)
        entry["lookups_per_us"] = lookups / entry["call_us"]["us"]
        try:
            entry["choices"] = time_beside({"default": hooked(0, True), "all_27_cells": hooked(0, False), "128_chunks": hooked(128, True), "32_chunks": hooked(32, True)}, a.reps)
            for max_chunks, skip in ((0, False), (128, True), (32, True)):  # and they change nothing
                hooked(max_chunks, skip)()
                assert torch.equal(out.sums[0], fused)
        finally:
            eng.debug_voxel_align(0, True)
        xyz_t = fx

        def whole():
            return eng.voxel_map_align(buf, params, xyz_t, None, fc, start, iterations=10, eps=(0.0, 0.0))

        def whole_unfused():
            sums_of = lambda cur, o: unfused(torch.from_numpy(cur[0]).cuda(), torch.from_numpy(o[0]).cuda().long())[0].cpu().numpy()[None]  # noqa: E731
            return sv.voxel_align_loop(sums_of, params, start, 10, 6, 6, (0.0, 0.0))

        got, want = whole(), whole_unfused()
        assert got.rounds == want["rounds"] == 10 and np.array_equal(got.poses, want["poses"]), "the two loops disagree on %s" % name
        entry["align_10_rounds_us"] = time_host(whole, max(a.reps // 3, 3))
        entry["start_error"], entry["end_error"] = ([float(v) for v in (np.degrees(np.arccos(np.clip((np.trace(p[:9].reshape(3, 3) @ truth[:9].reshape(3, 3).T) - 1) / 2, -1, 1))),
                                                                         np.linalg.norm(p[9:] - truth[9:]))] for p in (start[0], got.poses[0]))
        entry["pairs_per_round"] = got.pairs[:, 0].tolist()
        entry["unfused_us"] = time_events(unfused, max(a.reps // 3, 3))
        entry["unfused_align_10_rounds_us"] = time_host(whole_unfused, 3)
        entry["unfused_over_fused"] = entry["unfused_us"]["us"] / entry["call_us"]["us"]
        entry["unfused_over_fused_10_rounds"] = entry["unfused_align_10_rounds_us"]["us"] / entry["align_10_rounds_us"]["us"]
        entry["fused_is_faster"] = bool(entry["unfused_over_fused"] > 1)
        ch = entry["choices"]
        print("%s: %d rows, %d inside, %d pairs, %d look-ups; one round %.1f us (with the per-row outputs %.1f us), %.0f look-ups / us; beside each other: default %.1f, all 27 "
              "cells %.1f, 128 chunks %.1f, 32 chunks %.1f us; 10 rounds %.0f us, %.3f deg %.4f m -> %.4f deg %.4f m; unfused: one round %.0f us (%.1fx), 10 rounds %.0f us (%.1fx)"
              % (name, rows, entry["inside"], entry["pairs"], lookups, entry["call_us"]["us"], entry["call_per_row_us"]["us"], entry["lookups_per_us"], ch["default"]["us"],
                 ch["all_27_cells"]["us"], ch["128_chunks"]["us"], ch["32_chunks"]["us"], entry["align_10_rounds_us"]["us"], *entry["start_error"], *entry["end_error"],
                 entry["unfused_us"]["us"], entry["unfused_over_fused"], entry["unfused_align_10_rounds_us"]["us"], entry["unfused_over_fused_10_rounds"]), flush=True)
        res["runs"].append(entry)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
