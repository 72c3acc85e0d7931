#!/usr/bin/env python3
"""The connected components of the voxel map on a synthetic street (HIP events, median of --reps calls after warm-up, min / max beside the
median; one process).  The map, at --size metres: a ground plane of 800 x 800 cells and on it a grid of 66 x 66 blocks of 3 x 3 x 9 cells,
twelve cells apart - about a million voxels.  It is clustered at connectivity 26
  over all heights (mode 0): the ground joins everything, one component of a million voxels - every wavefront adds to one root and one row;
  over its own floor (mode 1: VoxelMap.flatten's floor plane, band 0.2 .. 2 m): the blocks alone, thousands of components.
Per run:
  (a) us per call of sv_voxel_clusters_device into pre-allocated outputs and workspace (1024 rows);
  (b) the kernels by difference, with sv_debug_voxel_clusters' stages: init alone, then with link, roots, count, scan, rank, stats, all;
  (c) the table look-ups of the link kernel - a member's half-neighbours inside the box - per microsecond of that kernel;
  (d) the two choices of the kernels, each against the default in the same run: one atomic per member instead of the wavefront's combine
      of equal destinations (roots and stats), and the link kernel without its path compression (link and roots);
  (e) the unfused form on the same device with torch ops: the members by a mask over the table, their keys sorted, a searchsorted per
      half-neighbour, least-label propagation (two scatter_reduce_("amin") per round) with pointer jumping to a fixed point, unique for the
      components, index_add_ for a sum.  Before anything is timed both forms must agree on members, components, the least keys, the voxels
      and the weight per component.
The yardstick is never the code under test.  Nothing is asserted about speed: fused_is_faster is reported.

    timeout -k 10 900 python tools/voxel_clusters_time.py [--reps 21] [--out profiles/voxel_clusters_time.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "low-cost-hardware-accelerated-vision-based-depth-perception-for-real-time-applications_amd"

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=21)
ap.add_argument("--size", type=float, default=0.2)
ap.add_argument("--side", type=int, default=800, help="cells of the ground plane per axis")
ap.add_argument("--out", default="")
a = ap.parse_args()

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
svmod = importlib.import_module(PKG + ".stereo_vision.sv")
L, U = eng.voxel_map_lib(), eng.voxel_clusters_lib()
size, side = a.size, a.side
ROWS, STAGES = 1024, ("init", "link", "roots", "count", "scan", "rank", "stats", "resolve")
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


# the street: cells, then a point in the middle of each
g = np.arange(side)
ground = np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3)
starts = np.arange(4, side - 4, 12)
block = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(1, 10), indexing="ij"), -1).reshape(-1, 3)
blocks = (np.stack(np.meshgrid(starts, starts, [0], indexing="ij"), -1).reshape(-1, 1, 3) + block).reshape(-1, 3)
cells = np.concatenate([ground, blocks])
cells = cells[np.random.default_rng(3).permutation(len(cells))]
cap = 65536
B = -(-len(cells) // cap)
xyz = np.zeros((B * cap, 3), np.float32)
xyz[:len(cells)] = (cells + 0.5) * size
counts = np.full(B, cap, np.int32)
counts[-1] = len(cells) - (B - 1) * cap
m = rigmod.VoxelMap((0.0, 0.0, 0.0), (side * size, side * size, 16 * size), size, len(cells) + len(cells) // 8)
m.update(torch.from_numpy(xyz.reshape(B, cap, 3)).cuda(), None, None, torch.from_numpy(counts).cuda(), np.tile(svmod.voxel_map_pose(0.0, 0.0, 0.0), (B, 1)))
n_voxels = m.stats()["claimed"]
assert n_voxels == len(cells) and not m.stats()["overflowed"]
params, buf = m.params, m.buffer
spec, nbytes = eng.voxel_map_spec(params), L.sv_voxel_map_bytes(params["capacity"])
slots = int(L.sv_voxel_map_slots(params["capacity"]))
table = buf[4:4 + 11 * slots].view(slots, 11)  # behind the head of 32 bytes: key, n, S[3], C[4], m, first_seq | last_seq << 32
flat_words = svmod.occupancy_map_params((0, int(np.ceil(side * size))), (0, int(np.ceil(side * size))), 2)
floor = m.flatten(flat_words, step=0.2, height=2.0, radius=2).floor
flat_c = eng._occupancy_map_struct(flat_words)
nc = torch.tensor(params["cells"], dtype=torch.int64, device="cuda")
as_t = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda")  # noqa: E731  (a tensor: torch divides by a Python number as a product with its reciprocal)
size_t, half_t, unit_t, ms_t = as_t(size), as_t(0.5), as_t(65536.0), as_t(float(flat_words["scale"]))
lo_t = [as_t(v) for v in params["lo"]]
res = {"size": size, "voxels_in_the_map": n_voxels, "capacity": params["capacity"], "table_slots": slots, "map_bytes": nbytes, "connectivity": 26, "rows": ROWS, "reps": a.reps, "runs": []}

for run_name, mode in (("all_heights_mode0", 0), ("over_the_floor_mode1", 1)):
    words = svmod.voxel_cluster_params(params, 26, 1, ROWS, mode)
    cspec = eng.voxel_cluster_spec(words)
    out = eng.voxel_map_clusters(buf, params, spec=words, flat_map=flat_words if mode else None, floor=floor if mode else None, sort=False)
    ws_bytes = out.workspace.numel() * 4

    def call():
        rc = U.sv_voxel_clusters_device(buf.data_ptr(), nbytes, ctypes.byref(spec), ctypes.byref(cspec), ctypes.byref(flat_c) if mode else None, floor.data_ptr() if mode else None,
                                        1, 1, 0, out.label.data_ptr(), out.rows.data_ptr(), out.info.data_ptr(), out.workspace.data_ptr(), ws_bytes, st)
        assert rc == 0, L.sv_last_error(None)

    def unfused():
        key, n = table[:, 0], table[:, 1]
        live = ((key != -1) & (n >= 1) & (table[:, 9] >= 1) & ((table[:, 10] >> 32) >= 0)).nonzero(as_tuple=True)[0]
        e = table[live]
        key, n = e[:, 0], e[:, 1]
        zq = ((key >> 40) & 0xFFFFF) * 256 + (torch.div(e[:, 4], n, rounding_mode="floor") >> 8)
        if mode == 0:
            member = (zq - words["z_ref_q"] >= words["h_lo_q"]) & (zq - words["z_ref_q"] < words["h_hi_q"])
        else:
            nf = n.double()
            gx, gy = (torch.floor((lo_t[k] + (((key >> (20 * k)) & 0xFFFFF).double() + (e[:, 2 + k].double() + half_t * nf) / (unit_t * nf)) * size_t) * ms_t) for k in range(2))
            inside = (gx >= flat_words["top"] - flat_words["rows"]) & (gx <= flat_words["top"] - 1) & (gy >= flat_words["left"] - flat_words["cols"]) & (gy <= flat_words["left"] - 1)
            r, c = torch.where(inside, flat_words["top"] - 1 - gx, 0).long(), torch.where(inside, flat_words["left"] - 1 - gy, 0).long()
            base = floor[r, c].long()
            h = zq - base
            member = inside & (base != -1) & (h >= words["h_lo_q"]) & (h < words["h_hi_q"])
        mk, by = torch.sort(key[member])
        weight = n[member][by]
        M = mk.numel()
        c3 = torch.stack([(mk >> (20 * k)) & 0xFFFFF for k in range(3)], -1)
        ei, ej, lookups = [], [], 0
        for d in svmod.VOXEL_CLUSTER_OFFSETS:
            nb = c3 + torch.tensor(d, dtype=torch.int64, device="cuda")
            ok = ((nb >= 0) & (nb < nc)).all(-1)
            nkey = nb[:, 0] | (nb[:, 1] << 20) | (nb[:, 2] << 40)
            at = torch.searchsorted(mk, nkey).clamp(max=max(M - 1, 0))
            hit = ok & (mk[at] == nkey)
            lookups = lookups + ok.sum()
            ei.append(hit.nonzero(as_tuple=True)[0]), ej.append(at[hit])
        ei, ej = torch.cat(ei), torch.cat(ej)
        lab = torch.arange(M, dtype=torch.int64, device="cuda")
        while True:
            new = lab.clone()
            new.scatter_reduce_(0, ei, lab[ej], "amin")
            new.scatter_reduce_(0, ej, lab[ei], "amin")
            while True:  # pointer jumping
                jumped = new[new]
                if torch.equal(jumped, new):
                    break
                new = jumped
            if torch.equal(new, lab):
                break
            lab = new
        roots, inv, voxels = torch.unique(lab, return_inverse=True, return_counts=True)
        return {"members": M, "least_key": mk[roots], "voxels": voxels, "n": torch.zeros_like(voxels).index_add_(0, inv, weight), "lookups": lookups}

    eng.debug_voxel_clusters(0, 0)
    call()
    slow = unfused()
    info = out.info.cpu().tolist()
    assert info[0] == slow["members"] and info[1] == slow["least_key"].numel(), "the fused and the unfused form disagree on members or components at %s" % run_name
    rows = out.rows[:min(info[2], ROWS)]
    at = torch.searchsorted(slow["least_key"], rows[:, 0].contiguous())
    for k, col in (("least_key", 0), ("voxels", 1), ("n", 2)):
        assert torch.equal(slow[k][at], rows[:, col]), "the fused and the unfused form disagree on %s at %s" % (k, run_name)
    lookups = int(slow["lookups"])
    entry = {"run": run_name, "words": words, "info": dict(zip(svmod.VOXEL_CLUSTER_INFO, info)), "link_lookups": lookups}

    def stage_times(flags):
        times = {}
        for k in list(range(1, 8)) + [0]:
            eng.debug_voxel_clusters(0, k | flags)
            times["upto_" + STAGES[k - 1 if k else 7]] = time_events(call, a.reps)
        eng.debug_voxel_clusters(0, 0)
        call()
        us = [times["upto_" + s]["us"] for s in STAGES]
        return times["upto_resolve"], {s + "_kernel_us": us[i] - (us[i - 1] if i else 0.0) for i, s in enumerate(STAGES)}

    entry["call_us"], kernels = stage_times(0)
    entry.update(kernels)
    entry["link_lookups_per_us"] = lookups / entry["link_kernel_us"]
    for name, flags in (("one_atomic_per_member", 16), ("no_path_compression", 32)):
        took, kern = stage_times(flags)
        entry[name] = {"call_us": took, "link_kernel_us": kern["link_kernel_us"], "roots_kernel_us": kern["roots_kernel_us"], "stats_kernel_us": kern["stats_kernel_us"]}
    entry["unfused_us"] = time_events(unfused, max(a.reps // 4, 3))
    entry["unfused_over_fused"] = entry["unfused_us"]["us"] / entry["call_us"]["us"]
    entry["fused_is_faster"] = bool(entry["unfused_over_fused"] > 1)
    print("%s: %d members, %d components, largest %d; call %.1f us (%s); %.0f look-ups / us; one atomic per member: call %.1f us (roots %.1f, stats %.1f); "
          "no path compression: call %.1f us (link %.1f, roots %.1f); unfused %.0f us (%.1fx)"
          % (run_name, info[0], info[1], info[5], entry["call_us"]["us"], ", ".join("%s %.1f" % (s, entry[s + "_kernel_us"]) for s in STAGES), entry["link_lookups_per_us"],
             entry["one_atomic_per_member"]["call_us"]["us"], entry["one_atomic_per_member"]["roots_kernel_us"], entry["one_atomic_per_member"]["stats_kernel_us"],
             entry["no_path_compression"]["call_us"]["us"], entry["no_path_compression"]["link_kernel_us"], entry["no_path_compression"]["roots_kernel_us"], entry["unfused_us"]["us"],
             entry["unfused_over_fused"]), flush=True)
    res["runs"].append(entry)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
