"""Inputs for a frame matched against the voxel map (group (R)) and an independent model of it: one Python loop per row and candidate over
a dict of the map's voxels, Python floats and ints only.  A frame is (xyz, n, counts) as voxel_map_match takes them; the maps come from
voxel_map_cases."""
import functools

import numpy as np

import voxel_map_cases as cases
from voxel_map_cases import IDENTITY

FIELDS = ("inside", "hits", "weight", "d2", "best", "best_weight", "best_d2")
DTYPES = dict(inside=np.int32, hits=np.int32, weight=np.int64, d2=np.int64, best=np.int32, best_weight=np.int64, best_d2=np.int64)


def same(got, want, fields=FIELDS):
    """Shape, dtype and bits of every field."""
    for k in fields:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.dtype != DTYPES[k] or a.tobytes() != b.tobytes():
            return False
    return True


def shifted(t, pose=IDENTITY):
    """`pose` with t added to its translation."""
    p = np.array(pose, np.float64)
    p[9:] += t
    return p


def model_match(sv, state, xyz, n, counts, poses, min_n=1, min_rows=1, since=0):
    """voxel_map_match's dict from a loop over frames, candidates and rows; a hit is a dict lookup of voxel_map_rows' keys."""
    params = state["params"]
    B, cap = xyz.shape[:2]
    poses = np.asarray(poses, np.float64).reshape(B, -1, 12)
    P = poses.shape[1]
    out = {k: np.zeros((B, P) if k in FIELDS[:4] else (B,), DTYPES[k]) for k in FIELDS}
    if state["overflowed"]:
        out["best"][:] = -1
        return out
    kept = set(sv.voxel_map_rows(state, min_n, min_rows, since, dtype="f64")["key"].tolist())
    mean = {int(k): [int(s) // int(w) for s in S] for k, w, S in zip(state["key"], state["n"], state["S"]) if int(k) in kept}
    for b in range(B):
        best = None
        for p in range(P):
            pose = [float(v) for v in poses[b, p]]
            inside = hits = weight = d2 = 0
            for i in range(max(0, min(int(counts[b]), cap))):
                w = 1 if n is None else int(n[b, i])
                r = cases.row_key(params, xyz[b, i], pose, w)
                if r is None:
                    continue
                inside += 1
                if r[0] in mean:
                    hits, weight = hits + 1, weight + w
                    d2 += sum((u - m) ** 2 for u, m in zip(r[1], mean[r[0]]))
            out["inside"][b, p], out["hits"][b, p], out["weight"][b, p], out["d2"][b, p] = inside, hits, weight, d2
            if best is None or (-weight, d2) < best[:2]:  # the first of the best
                best = (-weight, d2, p)
        out["best"][b], out["best_weight"][b], out["best_d2"][b] = best[2], -best[0], best[1]
    return out


def random_match(seed):
    """(params, calls, frame, poses, filters): voxel_map_cases.random_case(seed) as the map, its own rows as the frames to match - f32 and
    f64, with and without weights, counts of 0, -1 and above cap, rows that are not finite - and four candidates per frame: the frame's
    own pose, a shift by one cell, a shift by a fraction of a cell, and a pose with a word that is not finite."""
    params, calls = cases.random_case(seed)
    xyz, _, n, counts, poses = calls[0]
    size = params["size"]
    bad = shifted((0.0, 0.0, 0.0))
    bad[seed % 12] = (np.nan, np.inf)[seed % 2]
    cand = np.stack([np.stack([poses[b], shifted((size, 0.0, 0.0), poses[b]), shifted((0.0, -0.5 * size, 0.25 * size), poses[b]), bad]) for b in range(len(poses))])
    filters = (dict(), dict(min_rows=2), dict(min_n=3, since=0))[seed % 3]
    return params, calls, (xyz, n, counts), cand, filters


def filter_calls():
    """test_voxel_map.test_filters' three calls into BOX16: six voxels with n = 6, 12, 12, 8, 10, 12, m = 3, 6, 6, 4, 5, 6 and last_seq =
    2, 2, 1, 0, 0, 0 - and a frame of one row of weight 1 per voxel, in the voxels' order."""
    pts = cases.cell_points(np.repeat(cases.distinct_cells(6), [1, 2, 3, 4, 5, 6], 0))
    w = np.full(len(pts), 2, np.int32)
    calls = [cases.one_frame(pts, None, w), cases.one_frame(pts[:6], None, w[:6]), cases.one_frame(pts[:3], None, w[:3])]
    frame = (cases.cell_points(cases.distinct_cells(6), 0.25)[None], None, np.array([6], np.int32))
    return calls, frame


def ties_case():
    """(calls, xyz, counts, (off, exact, both, miss)): two voxels of BOX16 with mean offsets 32768, a frame of two rows, and four poses -
    `exact` puts row 0 on its voxel's mean and row 1 into an empty cell, `off` puts row 0 a quarter cell off in x, `both` lands both rows,
    half and a quarter cell off in z, `miss` lands none."""
    calls = [cases.one_frame(cases.cell_points([(3, 4, 5), (9, 9, 8)]))]
    xyz, counts = np.array([[[0.5, 0.5, 0.5], [6.5, 5.5, 4.25]]]), np.array([2], np.int32)
    return calls, xyz, counts, (shifted((3.25, 4.0, 5.0)), shifted((3.0, 4.0, 5.0)), shifted((3.0, 4.0, 4.5)), shifted((1.0, 1.0, 1.0)))


SCENE_BOX = dict(lo=(0.0, 0.0, 0.0), hi=(16.0, 16.0, 4.0), size=0.25, capacity=4096)
SCENE_TRUTH = np.array([7.0, 6.0, 0.5, 0.3])                    # where the vehicle stands: x, y, z, yaw
SCENE_GUESS = SCENE_TRUTH + np.array([0.25, -0.5, 0.25, -0.05])  # what its odometry says
SCENE_WINDOW = ((0.5, 0.5, 0.25, 0.1), (5, 5, 3, 5))             # steps of 0.25 m, 0.25 m, 0.25 m and 0.05 rad: 375 candidates


@functools.lru_cache(maxsize=None)
def scene():
    """(world float64 [1500,3], frame float64 [600,3]): an asymmetric scene - a floor patch and two walls of different extent - in the world,
    and 600 of its points as the vehicle at SCENE_TRUTH sees them: Pf = R^T (Pw - t)."""
    rng = np.random.default_rng(42)
    floor = np.stack([rng.uniform(2, 14, 700), rng.uniform(2, 12, 700), rng.uniform(0.05, 0.2, 700)], -1)
    wall_a = np.stack([rng.uniform(12.05, 12.2, 500), rng.uniform(3, 11, 500), rng.uniform(0.3, 3.0, 500)], -1)
    wall_b = np.stack([rng.uniform(4, 9, 300), rng.uniform(11.3, 11.45, 300), rng.uniform(0.3, 2.0, 300)], -1)
    world = np.concatenate([floor, wall_a, wall_b])
    pick = world[rng.permutation(len(world))[:600]]
    x, y, z, yaw = SCENE_TRUTH
    c, s = np.cos(yaw), np.sin(yaw)
    d = pick - np.array([x, y, z])
    frame = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], d[:, 2]], -1)
    world.setflags(write=False)
    frame.setflags(write=False)
    return world, frame
