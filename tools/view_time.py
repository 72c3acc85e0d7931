#!/usr/bin/env python3
"""The expected view of the world map from candidate poses on a KITTI map (HIP events, median of --reps samples).  The map is
frontier_time.py's: 2000 x 2000 cells at scale 10 - the CLI grid's - fused from the committed KITTI frames 0 .. 6 (tests/golden) along
that tool's drive.  The candidates are G points drawn (seeded) from the map's free cells, each at 16 headings, with a fan of 128 rays
over 90 degrees.  Per G in 64, 1024 and 4095 - 4096 x 16 would be one candidate above the 65535 a call takes - and per reach in 40 and
200 cells, alternated sample by sample in one process, after the results were asserted equal:
  (a) the call (engine.occupancy_view on tensors and a workspace made once: three kernels), the LDS bitmap sized by the call's reach
      (sv_debug_view's variant 0);
  (b) the same with the bitmap always 509 cells a side (variant 1);
  (c) the state-plane kernel alone (sv_debug_view's stages = 1);
  (d) the form a user of torch writes without the library, on the device: vectorised over candidates and rays, the steps k in a Python
      loop, the distinct cells by a scatter into a [K, window] bool tensor - in chunks of candidates that keep that tensor below 2 GiB.
Needs a GPU: there is nothing to time without one.

    python tools/view_time.py [--reps 5] [--out profiles/view_time.json]      (and the lines printed as <out>.txt)
"""
import argparse
import importlib
import json
import math
import os
import sys

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "low-cost-hardware-accelerated-vision-based-depth-perception-for-real-time-applications_amd"

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--groups", type=int, nargs="*", default=[64, 1024, 4095])
ap.add_argument("--reaches", type=int, nargs="*", default=[40, 200])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "view_time.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("view_time.py: no GPU - nothing is measured, profiles/view_time.* stay as they are")

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
sv = importlib.import_module(PKG + ".stereo_vision.sv")
W, H = 1242, 375
GOLDEN = os.path.join(ROOT, "tests", "golden")
LINES = []
KEYS = ("counts", "end_cells", "status", "best", "best_score")
HEADINGS, RAYS, FOV = 16, 128, math.pi / 2


def say(text):
    LINES.append(text)
    print(text, flush=True)


def png(name):
    return np.asarray(Image.open(os.path.join(GOLDEN, name)))


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
words = world.words
ROWS, COLS, TOP, LEFT, MS = words["rows"], words["cols"], words["top"], words["left"], float(words["scale"])
OCCUPIED, FREE = words["l_occ"], -words["l_free"]
free_cells = np.argwhere(world.state().cpu().numpy() == 1)
Xc, Yc = sv.occupancy_map_centres(words)
rng = np.random.default_rng(21)


def sample(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def time_alternated(fns, reps):
    """{name: median us per call}; one sample of each in turn, reps times over, after one call of each to warm up."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ts[k].append(sample(fn))
    return {k: float(np.median(v)) for k, v in ts.items()}


def torch_view(logodds, last_seen, poses, ends, reach, max_unknown=0):
    """occupancy_view as a user of torch writes it -> the five tensors."""
    dev = logodds.device
    L = logodds.to(torch.int32)
    S = torch.where(last_seen >= 0, torch.where(L >= OCCUPIED, 2, torch.where(L <= FREE, 1, 0)), 0).to(torch.uint8)
    G, P = poses.shape[:2]
    K, R, side = G * P, ends.shape[0], 2 * reach + 1
    counts = torch.zeros((K, 3), dtype=torch.int32, device=dev)
    end_cells = torch.full((K, R, 2), -1, dtype=torch.int16, device=dev)
    status = torch.full((K, R), 5, dtype=torch.uint8, device=dev)
    score = torch.full((K,), -1, dtype=torch.int32, device=dev)
    flat = poses.reshape(K, 4)
    chunk = max(1, min(K, (2 << 30) // (side * side)))
    for k0 in range(0, K, chunk):
        p = flat[k0:k0 + chunk]
        n_c = p.shape[0]
        tx, ty, c, s = (p[:, i:i + 1] for i in range(4))
        gx0, gy0 = torch.floor(tx * MS), torch.floor(ty * MS)
        origin = torch.isfinite(p).all(1, keepdim=True) & (gx0 >= TOP - ROWS) & (gx0 <= TOP - 1) & (gy0 >= LEFT - COLS) & (gy0 <= LEFT - 1)
        Xw, Yw = (c * ends[:, 0] - s * ends[:, 1]) + tx, (s * ends[:, 0] + c * ends[:, 1]) + ty
        gx1, gy1 = torch.floor(Xw * MS), torch.floor(Yw * MS)
        ddr, ddc = gx0 - gx1, gy0 - gy1
        valid = origin & torch.isfinite(gx1) & torch.isfinite(gy1) & (ddr.abs() <= reach) & (ddc.abs() <= reach)
        zero = torch.zeros_like(ddr)
        dr, dc = torch.where(valid, ddr, zero).long(), torch.where(valid, ddc, zero).long()
        r0 = torch.where(origin, TOP - 1 - gx0, torch.zeros_like(gx0)).long()
        c0 = torch.where(origin, LEFT - 1 - gy0, torch.zeros_like(gy0)).long()
        n = torch.maximum(dr.abs(), dc.abs())
        n1 = n.clamp(min=1)
        window = torch.zeros((n_c, side * side), dtype=torch.bool, device=dev)
        window[:, reach * side + reach] = valid.any(1)
        alive = valid.clone()
        st = torch.where(valid, 0, 5).to(torch.uint8)
        er, ec = r0.expand(-1, R).clone(), c0.expand(-1, R).clone()
        pr, pc = er.clone(), ec.clone()
        unknown = torch.zeros((n_c, R), dtype=torch.int32, device=dev)
        rows_k = torch.arange(n_c, device=dev)[:, None].expand(-1, R)

        def state_at(r, cc):
            inside = (r >= 0) & (r < ROWS) & (cc >= 0) & (cc < COLS)
            return torch.where(inside, S[r.clamp(0, ROWS - 1), cc.clamp(0, COLS - 1)], 2), inside

        for k in range(1, reach + 1):
            active = alive & (n >= k)
            if not bool(active.any()):  # the wait a user of torch pays to stop early
                break
            r = r0 + torch.div(2 * k * dr + n, 2 * n1, rounding_mode="floor")
            cc = c0 + torch.div(2 * k * dc + n, 2 * n1, rounding_mode="floor")
            here, inside = state_at(r, cc)
            edge = active & ~inside
            side_a, _ = state_at(pr, cc)
            side_b, _ = state_at(r, pc)
            corner = active & inside & (r != pr) & (cc != pc) & (side_a == 2) & (side_b == 2)
            visible = active & inside & ~corner
            at = (r - r0 + reach) * side + (cc - c0 + reach)
            window[rows_k[visible], at[visible]] = True
            hit = visible & (here == 2)
            unknown += (visible & (here == 0)).int()
            spent = visible & (here == 0) & (unknown == max_unknown) if max_unknown > 0 else torch.zeros_like(hit)
            st = torch.where(edge, 2, torch.where(corner, 3, torch.where(hit, 1, torch.where(spent, 4, st)))).to(torch.uint8)
            er, ec = torch.where(visible, r, er), torch.where(visible, cc, ec)
            pr, pc = torch.where(visible, r, pr), torch.where(visible, cc, pc)
            alive = alive & ~(edge | corner | hit | spent)
        span = torch.arange(-reach, reach + 1, device=dev)
        patch = S[(r0 + span[None, :]).clamp(0, ROWS - 1)[:, :, None], (c0 + span[None, :]).clamp(0, COLS - 1)[:, None, :]].reshape(n_c, side * side)
        for v in range(3):
            counts[k0:k0 + n_c, v] = (window & (patch == v)).sum(1).int()
        score[k0:k0 + n_c] = torch.where(origin[:, 0], counts[k0:k0 + n_c, 0], -1)
        status[k0:k0 + n_c] = st
        end_cells[k0:k0 + n_c] = torch.where(valid[..., None], torch.stack([er, ec], -1), -1).to(torch.int16)
    score = score.reshape(G, P)
    best_score, best = score.max(1)
    best = (score == best_score[:, None]).int().argmax(1)  # the first of the largest
    return {"counts": counts.reshape(G, P, 3), "end_cells": end_cells.reshape(G, P, R, 2), "status": status.reshape(G, P, R), "best": best.int(), "best_score": best_score.int()}


res = {"map": dict(rows=ROWS, cols=COLS, scale=MAP["scale"]), "headings": HEADINGS, "rays": RAYS, "fov_deg": 90.0, "reps": a.reps, "points": []}
for G in a.groups:
    at = free_cells[rng.choice(len(free_cells), G, replace=len(free_cells) < G)]
    poses = torch.from_numpy(sv.view_headings(np.stack([Xc[at[:, 0]], Yc[at[:, 1]]], 1), HEADINGS)).cuda()
    for reach in a.reaches:
        ends_np, got_reach = sv.view_rays(FOV, RAYS, (reach - 1) / MAP["scale"], MAP["scale"])
        assert got_reach == reach
        ends = torch.from_numpy(ends_np).cuda()
        out = eng.occupancy_view(world.logodds, world.last_seen, words, poses, ends, reach, OCCUPIED, FREE)
        ws = out.workspace

        def call(variant, stages=3):
            def run():
                eng.debug_view(variant, stages)
                eng.occupancy_view(world.logodds, world.last_seen, words, poses, ends, reach, OCCUPIED, FREE, out=out, workspace=ws)
                eng.debug_view(0, 3)
            return run

        runs = {}
        for variant in (0, 1):
            for t in (out.counts, out.end_cells, out.status, out.best, out.best_score):
                t.fill_(99)
            call(variant)()
            torch.cuda.synchronize()
            runs[variant] = {k: getattr(out, k).cpu().numpy().copy() for k in KEYS}
        assert all(np.array_equal(runs[0][k], runs[1][k]) for k in KEYS), "the variants differ at G %d reach %d" % (G, reach)
        form = torch_view(world.logodds, world.last_seen, poses, ends, reach)
        assert all(np.array_equal(runs[0][k], form[k].cpu().numpy()) for k in KEYS), "the torch form differs from the kernels at G %d reach %d" % (G, reach)
        t = time_alternated({"call": call(0), "full_window": call(1), "state": call(0, 1), "torch": lambda: torch_view(world.logodds, world.last_seen, poses, ends, reach)}, a.reps)
        unknown = runs[0]["counts"][..., 0]
        row = {"groups": G, "candidates": G * HEADINGS, "reach": reach, "call_us": t["call"], "full_window_us": t["full_window"], "full_window_over_call": t["full_window"] / t["call"],
               "state_us": t["state"], "state_share": t["state"] / t["call"], "torch_us": t["torch"], "torch_over_call": t["torch"] / t["call"],
               "mean_unknown_cells": float(unknown.mean()), "mean_cells_seen": float(runs[0]["counts"].sum(-1).mean()), "torch_equals_kernels": True}
        res["points"].append(row)
        say("G %4d x %d, reach %3d: call %.0f us; bitmap always 509 wide %.0f us (x%.2f); state plane alone %.0f us (%.0f %% of the call); torch form %.0f us (x%.1f); "
            "%.0f cells seen per candidate, %.0f of them unknown" % (G, HEADINGS, reach, row["call_us"], row["full_window_us"], row["full_window_over_call"], row["state_us"],
                                                                  100 * row["state_share"], row["torch_us"], row["torch_over_call"], row["mean_cells_seen"], row["mean_unknown_cells"]))
        say("  the call is faster than the torch form: %s; sizing the bitmap by reach pays: %s" % ("met" if row["torch_over_call"] > 1 else "missed",
                                                                                               "met" if row["full_window_over_call"] > 1 else "missed"))

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
    f.write("\n".join(LINES) + "\n")
