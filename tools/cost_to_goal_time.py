#!/usr/bin/env python3
"""The cost-to-goal field of the world map and the routes through it on a KITTI map (HIP events, median of --reps samples).  The map is
clearance_time.py's: 2000 x 2000 cells at scale 10 (x -40..160, y -100..100), fused from the committed KITTI frames 0 .. 6 (tests/golden)
along that tool's drive; the clearance field has R = 10 cells, cells within 5 of an obstacle are blocked and cells within 10 pay 5 per cell
of the difference.  Two goals, each a field of its own: one near the drive and one in the map's far corner.
  (a) engine.occupancy_cost_to_goal - the whole call, its waits for the 16 bytes of info after every round of 16 sweeps included - with the
      tiles the dirty bytes name (variant 0) and with every tile in every sweep (sv_debug_cost_to_goal's variant 1), alternated sample by
      sample; the sweeps, and the tiles run against tiles x sweeps;
  (b) the form a user writes without it, in the same process and alternated with (a), after asserting that it yields the same bits: a
      whole-map Jacobi relaxation, torch.minimum over the eight shifted views, until a look every 16 iterations finds nothing changed;
  (c) sv_cost_cells_device, and sv_cost_routes_device for K = 1, 64 and 4096 routes of at most 4096 cells on the far goal's field.
Needs a GPU: there is nothing to time without one.

    python tools/cost_to_goal_time.py [--reps 5] [--out profiles/cost_to_goal_time.json]      (and the lines printed as <out>.txt)
"""
import argparse
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--routes", default="1,64,4096")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cost_to_goal_time.json"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("cost_to_goal_time.py: no GPU - nothing is measured, profiles/cost_to_goal_time.* stay as they are")

rigmod = importlib.import_module(PKG + ".rig")
eng = importlib.import_module(PKG + ".engine")
sv = importlib.import_module(PKG + ".stereo_vision.sv")
L = eng.cost_lib()
W, H = 1242, 375
G = os.path.join(ROOT, "tests", "golden")
LINES = []


def say(text):
    LINES.append(text)
    print(text, flush=True)


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
RADIUS, BLOCK, SOFT, WEIGHT, CAPACITY = 10, 5, 10, 5, 4096
INF = sv.COST_INF


def drive(n):
    yaw = STEP_RAD * np.arange(n)
    x = np.concatenate([[0.0], np.cumsum(STEP_M * np.cos(yaw))[:-1]])
    y = np.concatenate([[0.0], np.cumsum(STEP_M * np.sin(yaw))[:-1]])
    return sv.occupancy_pose(x, y, yaw)


world = rigmod.OccupancyMap(**MAP)
world.update(occ, drive(7))
words = world.words
ROWS, COLS = words["rows"], words["cols"]
TILES = ((ROWS + 63) // 64) * ((COLS + 63) // 64)
d2 = world.clearance(RADIUS / MAP["scale"])
pen = torch.empty((ROWS, COLS), dtype=torch.uint8, device="cuda")
cost = torch.empty((ROWS, COLS), dtype=torch.int32, device="cuda")
STREAM = torch.cuda.current_stream().cuda_stream


def cells_call():
    eng.cost_cells(d2, RADIUS, BLOCK * BLOCK, SOFT, WEIGHT, out=pen)


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


cells_call()
torch.cuda.synchronize()
pen_np = pen.cpu().numpy()
assert np.array_equal(pen_np, sv.cost_cells(d2.cpu().numpy(), BLOCK * BLOCK, SOFT, WEIGHT, radius=RADIUS)), "cost_cells differs from its definition"
cells_us = time_alternated({"cells": cells_call}, 20)["cells"]
res = {"map": dict(rows=ROWS, cols=COLS, scale=MAP["scale"]), "radius": RADIUS, "block_cells": BLOCK, "soft": SOFT, "weight": WEIGHT, "blocked_cells": int((pen_np == 255).sum()),
       "penalised_cells": int(((pen_np > 0) & (pen_np < 255)).sum()), "tiles": TILES, "reps": a.reps, "cost_cells_us": cells_us, "field": [], "routes": []}
say("map %d x %d (%d tiles): %d blocked cells, %d penalised; cost_cells %.1f us" % (ROWS, COLS, TILES, res["blocked_cells"], res["penalised_cells"], cells_us))


def free_cell_near(r, c):
    """The first free cell at or after (r, c) in row-major order - a goal must not sit on a blocked cell."""
    flat = np.flatnonzero(pen_np.reshape(-1)[r * COLS + c:] != 255)[0] + r * COLS + c
    return int(flat // COLS), int(flat % COLS)


near = free_cell_near(*[int(v) for v in sv.occupancy_cells_of(words, (30.0, 0.0))])
far = free_cell_near(ROWS - 8, COLS - 64)
P32 = pen.to(torch.int32)
FREE = torch.zeros((ROWS + 2, COLS + 2), dtype=torch.bool, device="cuda")
FREE[1:-1, 1:-1] = pen != 255


def view(t, dr, dc):
    return t[1 + dr:1 + dr + ROWS, 1 + dc:1 + dc + COLS]


def torch_field(goal, look=16):
    """(int32 [rows,cols], iterations): whole-map Jacobi relaxations from the all-COST_INF start until nothing changes."""
    inf = torch.full((), INF, dtype=torch.int32, device="cuda")
    ok = [view(FREE, 0, 0) & view(FREE, dr, dc) & view(FREE, dr, 0) & view(FREE, 0, dc) for dr, dc in sv.COST_MOVES]
    big = torch.full((ROWS + 2, COLS + 2), INF, dtype=torch.int32, device="cuda")
    now = view(big, 0, 0)
    now[goal[0], goal[1]] = 0
    n = 0
    while True:
        best = now.clone()
        for k, (dr, dc) in enumerate(sv.COST_MOVES):
            b = view(big, dr, dc)
            best = torch.minimum(best, torch.where(ok[k] & (b != inf), b + ((10 if k < 4 else 14) + P32), inf))  # a wrapped sum is masked
        n += 1
        if n % look == 0 and torch.equal(best, now):  # the one wait, as the call's info every 16 sweeps
            return best, n
        now.copy_(best)


ws = None
for name, goal in (("near the drive", near), ("far corner", far)):
    goals = np.array([goal], np.int32)
    row = {"goal": name, "goal_cell": list(goal)}
    runs = {}
    for variant in (0, 1):
        counters = torch.zeros(2, dtype=torch.int64, device="cuda")
        assert eng.debug_cost_to_goal(variant, counters) == 0
        r = eng.occupancy_cost_to_goal(pen, goals, max_sweeps=ROWS * COLS, out=cost, workspace=ws)
        torch.cuda.synchronize()
        eng.debug_cost_to_goal(0, None)
        ws = r.workspace
        runs[variant] = (r.sweeps, r.converged, cost.clone(), counters.cpu().numpy().tolist())
    assert runs[0][1] and runs[1][1] and runs[0][0] == runs[1][0] and torch.equal(runs[0][2], runs[1][2]), "the variants differ"
    want, iterations = torch_field(goal)
    assert torch.equal(want, runs[0][2]), "the torch form differs from the kernels for the goal %s" % name
    sweeps = runs[0][0]
    launched = 16 * ((sweeps + 15) // 16)
    assert runs[1][3][0] == TILES * launched

    def call(variant):
        def run():
            eng.debug_cost_to_goal(variant, None)
            eng.occupancy_cost_to_goal(pen, goals, max_sweeps=ROWS * COLS, out=cost, workspace=ws)
            eng.debug_cost_to_goal(0, None)
        return run

    t = time_alternated({"dirty": call(0), "all": call(1), "torch": lambda: torch_field(goal)}, a.reps)
    row.update({"sweeps": sweeps, "sweeps_launched": launched, "reachable_cells": int((want != INF).sum().item()), "max_cost": int(want[want != INF].max().item()),
                "tiles_run": runs[0][3][0], "inner_iterations": runs[0][3][1], "tiles_x_sweeps": TILES * sweeps, "tiles_run_share": runs[0][3][0] / (TILES * sweeps),
                "tiles_run_all": runs[1][3][0], "inner_iterations_all": runs[1][3][1], "call_us": t["dirty"], "all_tiles_us": t["all"], "all_over_call": t["all"] / t["dirty"],
                "torch_iterations": iterations, "torch_us": t["torch"], "torch_over_call": t["torch"] / t["dirty"], "torch_equals_kernels": True})
    res["field"].append(row)
    say("goal %-14s (%4d,%4d): %d sweeps (%d launched), tiles run %d of %d (%.3f), %d inner iterations; call %.0f us, every tile %.0f us (x%.2f); torch %d iterations %.0f us (x%.1f)"
        % (name, goal[0], goal[1], sweeps, launched, row["tiles_run"], row["tiles_x_sweeps"], row["tiles_run_share"], row["inner_iterations"], row["call_us"], row["all_tiles_us"],
           row["all_over_call"], iterations, row["torch_us"], row["torch_over_call"]))

# ---- routes down the far goal's field, from cells spread over what reaches it
field = runs[0][2]
field_np = field.cpu().numpy()
reach = np.flatnonzero(field_np.reshape(-1) != INF)
rng = np.random.default_rng(5)
for K in [int(v) for v in a.routes.split(",")]:
    pick = rng.choice(reach, K, replace=False)
    starts_np = np.stack([pick // COLS, pick % COLS], -1).astype(np.int32)
    starts = torch.from_numpy(starts_np).cuda()
    cells = torch.empty((K, CAPACITY, 2), dtype=torch.int16, device="cuda")
    length, status = (torch.empty(K, dtype=torch.int32, device="cuda") for _ in range(2))

    def call():
        rc = L.sv_cost_routes_device(field.data_ptr(), pen.data_ptr(), ROWS, COLS, starts.data_ptr(), K, CAPACITY, cells.data_ptr(), length.data_ptr(), status.data_ptr(), STREAM)
        assert rc == 0, L.sv_last_error(None)

    call()
    torch.cuda.synchronize()
    check = min(K, 8)  # the definition walks in Python: a few routes of each batch
    want = sv.cost_routes(field_np, pen_np, starts_np[:check], CAPACITY)
    assert np.array_equal(cells[:check].cpu().numpy(), want["cells"]) and np.array_equal(length[:check].cpu().numpy(), want["length"]) and \
        np.array_equal(status[:check].cpu().numpy(), want["status"]), "the route kernel differs from its definition at K = %d" % K
    t = time_alternated({"call": call}, 20)
    lengths = length.cpu().numpy()
    row = {"routes": K, "capacity": CAPACITY, "call_us": t["call"], "mean_length": float(lengths.mean()), "max_length": int(lengths.max()),
           "status_counts": np.bincount(status.cpu().numpy(), minlength=5).tolist()}
    res["routes"].append(row)
    say("K=%-4d capacity %d: call %.1f us; lengths mean %.0f, max %d; statuses 0..4 %s" % (K, CAPACITY, row["call_us"], row["mean_length"], row["max_length"], row["status_counts"]))

os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
with open(os.path.splitext(a.out)[0] + ".txt", "w") as f:
    f.write("\n".join(LINES) + "\n")
