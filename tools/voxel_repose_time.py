#!/usr/bin/env python3
"""A voxel map re-posed under per-frame rigid corrections on a synthetic street (HIP events, medians of --reps calls after warm-up, min /
max beside the median, the variants in alternating rounds; one process, every buffer allocated before anything is timed).  The map, at
--size metres, is tools/voxel_align_time.py's street - a ground plane of 800 x 800 cells and 66 x 66 blocks on it, about a million voxels -
inserted as frames of 1 024 rows, so that last_seq runs over about a thousand frames.  sv_voxel_repose_device from that map into an empty
table of the same box and capacity:
  identity   one correction, the identity: every voxel lands in its own cell, no two in one;
  spread     K = 1 000 corrections, small rigid motions that grow along the drive, as loop_spread gives them: a gather of 96 bytes per
             voxel from a table of 96 KB, some voxels share a cell;
  fold       one correction that scales x by a tenth: ten source voxels per destination cell, the atomics contended;
beside sv_voxel_map_carry_device of the same map into the same table in the same rounds - the floor: the same walk with plain stores -, the
destination's clear, timed alone and subtracted from each, and the same definition in torch ops on the same device (the table's rows, the
transform, unique, index_add_, scatter_reduce_), which must equal the kernel's table bit for bit before anything is timed.  Nothing is
asserted about speed.

    timeout -k 10 900 python tools/voxel_repose_time.py [--reps 21] [--out profiles/voxel_repose_time.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import voxel_align_time as street  # noqa: E402 (the map's cells and the timers)

PKG = street.PKG
ROWS = 1024  # rows per frame of the feed


def table_of(buf, slots):
    return buf[4:4 + 11 * slots].view(slots, 11)  # behind the head of 32 bytes: key, n, S[3], C[4], m, first_seq | last_seq << 32


def torch_repose(src_table, params, corr, seq0):
    """The definition with torch ops, into an empty map of the same params: -> (the entries in ascending key [V,11], carried, outside)."""
    dev = src_table.device
    f = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)  # noqa: E731  (tensors: torch divides by a Python number as a product with its reciprocal)
    lo, hi, size, cells = f(params["lo"]), f(params["hi"]), f(params["size"]), torch.tensor(params["cells"], dtype=torch.int64, device=dev)
    e = src_table[(src_table[:, 0] != -1) & (src_table[:, 1] >= 1) & (src_table[:, 9] >= 1) & ((src_table[:, 10] >> 32) >= 0)]
    key, n = e[:, 0], e[:, 1]
    c = torch.stack([(key >> (20 * k)) & 0xFFFFF for k in range(3)], -1)
    nf = n.double()[:, None]
    p = lo + (c.double() + (e[:, 2:5].double() + f(0.5) * nf) / (f(65536.0) * nf)) * size
    w = corr[torch.clamp((e[:, 10] >> 32) - seq0, 0, corr.shape[0] - 1)]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    Pw = torch.stack([((w[:, 3 * k] * x + w[:, 3 * k + 1] * y) + w[:, 3 * k + 2] * z) + w[:, 9 + k] for k in range(3)], -1)
    keep = ((lo < Pw) & (Pw < hi)).all(-1)
    e, Pw, n = e[keep], Pw[keep], n[keep]
    t = (Pw - lo) / size
    c = torch.minimum(t.long(), cells - 1)
    u = torch.clamp(((t - c.double()) * f(65536.0)).long(), max=65535)
    moved = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
    ukey, inv = torch.unique(moved, return_inverse=True)
    V = ukey.numel()
    sums = torch.zeros((V, 9), dtype=torch.int64, device=dev)
    sums.index_add_(0, inv, torch.cat([n[:, None], n[:, None] * u, e[:, 5:10]], 1))
    first = torch.full((V,), 2 ** 62, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, e[:, 10] & 0xFFFFFFFF, "amin")
    last = torch.full((V,), -1, dtype=torch.int64, device=dev).scatter_reduce_(0, inv, e[:, 10] >> 32, "amax")
    return torch.cat([ukey[:, None], sums, (first | (last << 32))[:, None]], 1), int(keep.sum()), int((~keep).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--size", type=float, default=0.2)
    ap.add_argument("--side", type=int, default=800, help="cells of the ground plane per axis")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    eng = importlib.import_module(PKG + ".engine")
    sv = importlib.import_module(PKG + ".stereo_vision.sv")
    L, C, R = eng.voxel_map_lib(), eng.voxel_carry_lib(), eng.voxel_repose_lib()
    size, side = a.size, a.side
    st = torch.cuda.current_stream().cuda_stream

    cells = street.street_cells(side)
    B = -(-len(cells) // ROWS)
    xyz = np.zeros((B * ROWS, 3), np.float32)
    xyz[:len(cells)] = (cells + np.random.default_rng(5).uniform(0.1, 0.9, cells.shape)) * size
    counts = np.full(B, ROWS, np.int32)
    counts[-1] = len(cells) - (B - 1) * ROWS
    params = sv.voxel_map_params((0.0, 0.0, 0.0), (side * size, side * size, 16 * size), size, len(cells) + len(cells) // 8)
    spec, nbytes = eng.voxel_map_spec(params), L.sv_voxel_map_bytes(params["capacity"])
    slots = int(L.sv_voxel_map_slots(params["capacity"]))
    src, dst = eng.voxel_map_new(params), eng.voxel_map_new(params)
    eng.voxel_map_insert(src, params, torch.from_numpy(xyz.reshape(B, ROWS, 3)).cuda(), None, None, torch.from_numpy(counts).cuda(), np.tile(sv.voxel_map_pose(0.0, 0.0, 0.0), (B, 1)))
    V = eng.voxel_map_stats(src)[0]
    assert V == len(cells) and not eng.voxel_map_stats(src)[2]

    # the corrections
    K = 1000
    f = np.arange(K) / (K - 1.0)
    xi = np.array([0.0, 0.0, 0.004, 0.9, -0.6, 0.05])  # what a loop of this length gathers: 0.23 degrees and a metre
    mid = sv.voxel_map_pose(0.5 * side * size, 0.5 * side * size, 0.0)
    spread = np.array([sv._pose_mul(mid, sv._pose_mul(sv.pose_exp(fk * xi), sv._pose_inv(mid))) for fk in f])  # about the middle of the map
    fold = np.array([[0.1, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0.45 * side * size, 0, 0]])
    corrs = {"identity": torch.from_numpy(sv.flow_identity(1)).cuda(), "spread": torch.from_numpy(spread).cuda(), "fold": torch.from_numpy(fold).cuda()}
    stats = torch.zeros(4, dtype=torch.int64, device="cuda")

    def clear():
        assert L.sv_voxel_map_clear_device(dst.data_ptr(), nbytes, ctypes.byref(spec), st) == 0

    def carry():
        clear()
        assert C.sv_voxel_map_carry_device(dst.data_ptr(), nbytes, ctypes.byref(spec), src.data_ptr(), nbytes, ctypes.byref(spec), 0, 0, 0, 1, 1, 0, stats.data_ptr(), st) == 0

    def repose(name):
        clear()
        c = corrs[name]
        assert R.sv_voxel_repose_device(dst.data_ptr(), nbytes, ctypes.byref(spec), src.data_ptr(), nbytes, ctypes.byref(spec), c.data_ptr(), int(c.shape[0]), 0, 1, 1, 0,
                                        stats.data_ptr(), st) == 0

    # the torch form and the kernel agree bit for bit, variant by variant
    counts_of = {}
    for name, c in corrs.items():
        repose(name)
        got = table_of(dst, slots)
        got = got[got[:, 0] != -1]
        got = got[torch.sort(got[:, 0]).indices]
        want, carried, outside = torch_repose(table_of(src, slots), params, c, 0)
        said = stats.cpu().tolist()
        assert said[0] == carried and said[2] == outside and said[3] == want.shape[0] and torch.equal(got, want), "the torch form differs under %s" % name
        counts_of[name] = dict(zip(sv.VOXEL_CARRY_STATS, said))
    del got, want
    torch.cuda.empty_cache()

    fns = {"clear": clear, "carry": carry}
    fns.update({name: (lambda name=name: repose(name)) for name in corrs})
    t = street.time_beside(fns, a.reps)
    res = {"size": size, "voxels_in_the_map": V, "capacity": params["capacity"], "table_slots": slots, "map_bytes": nbytes, "frames": B, "corrections": K, "reps": a.reps,
           "entry_bytes": 88, "clear_us": t["clear"], "torch_form_is_bit_equal": True, "variants": {}}
    clear_us = t["clear"]["us"]
    carry_us = t["carry"]["us"] - clear_us
    res["carry"] = dict(t["carry"], us_without_clear=carry_us, voxels_per_us=V / carry_us)
    for name, c in corrs.items():
        us = t[name]["us"] - clear_us
        torch_t = street.time_events(lambda c=c: torch_repose(table_of(src, slots), params, c, 0), max(a.reps // 3, 3))
        res["variants"][name] = dict(t[name], us_without_clear=us, voxels_per_us=V / us, over_carry=us / carry_us, counts=counts_of[name], torch_form_us=torch_t,
                                     torch_form_over_kernel=torch_t["us"] / us)
        print("%-8s %8.1f us (%.1f voxels / us), %.2fx the carry (%.1f us), torch form %.0f us (%.1fx); %s" % (
            name, us, V / us, us / carry_us, carry_us, torch_t["us"], torch_t["us"] / us, counts_of[name]), flush=True)
    res["not_measured"] = ["a merge of equal destination cells in front of the atomics (wave_run): equal cells do not sit in neighbouring lanes of a hashed table",
                           "other voxel sizes and table fills", "a destination that already holds the voxels", "counters (rocprofv3 --pmc)"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
