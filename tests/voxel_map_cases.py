"""Inputs for the world-fixed voxel map (group (Q)) and an independent model of it: one Python loop per row over a dict, Python floats and
ints only.  A case is (params, calls): params a dict of lo, hi, size, capacity and calls a list of (xyz, color, n, counts, poses) - numpy
arrays as voxel_map_insert takes them, one call per update.  The painted cases build wavefront layouts lane by lane: a frame's row i is
lane i % 64 of wavefront i // 64, and four wavefronts make a workgroup."""
import math
import os
import re

import numpy as np

IDENTITY = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
QUARTER = np.array([0.0, -1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0])  # (c, s) = (0, 1), exact
FIELDS = ("xyz", "color", "cell", "n", "m", "first_seq", "last_seq", "key")
BOX16 = dict(lo=(0.0, 0.0, 0.0), hi=(16.0, 16.0, 16.0), size=1.0, capacity=512)  # 16 cells per axis, a table of 1024 slots
MAP_STAGES = ("voxel_map", "voxel_match", "voxel_carry", "voxel_carve")  # each a <stage>_kernels.hip and a <stage>.cpp
# The texts that define the map's table and cell rules, and how often csrc/voxel_map_table.h states each: once, but for the probe loop's
# line, which its read-only probe (vmap_find) and its claiming probe (vmap_claim) have each.  No other file of the stages states one,
# but for the insert's copy of the claiming probe (voxel_map_kernels.hip: vmap_add), which test_voxel_map.py holds against the header.
PROBE_LOOP = "for (uint32_t probe = 0; probe <= last; probe++, h = (h + 1) & last) {"
TABLE_TEXTS = {
    "0x9E3779B97F4A7C15": 1,
    "VMAP_EMPTY = ~0ull": 1,
    PROBE_LOOP: 2,
    "__hip_atomic_load(head + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)": 1,
    "const double P = ((pose[3 * k] * x + pose[3 * k + 1] * y) + pose[3 * k + 2] * z) + pose[9 + k];": 1,
    "keep = keep && a.lo[k] < P && P < a.hi[k];": 1,
    "t = keep ? (P - a.lo[k]) / a.size : 0.0;": 1,
    "c = (long long)t;": 1,
    "if (c > a.nc[k] - 1) c = a.nc[k] - 1;": 1,
    "const long long f = (long long)((t - (double)c) * 65536.0);": 1,
    "return f > 65535 ? 65535 : f;": 1,
    "return cnt < cap ? cnt : cap;": 1,
}


def squeeze(text):
    return re.sub(r"\s+", "", text)


def check_map_table(build):
    """The rules that the stages of the map share are defined once, in csrc/voxel_map_table.h.  Returns the squeezed text of the header."""
    assert "voxel_map_table.h" in build.HEADERS
    read = lambda name: open(os.path.join(build.CSRC, name)).read()  # noqa: E731
    header = squeeze(read("voxel_map_table.h"))
    for stage in MAP_STAGES:
        kernels = read(stage + "_kernels.hip")
        assert '#include "voxel_map_table.h"' in kernels, stage
        # an entry's words go by their names (VMAP_N ...), never by a bare number
        assert re.findall(r"(?<!int )\b[ed]\[\d", re.sub(r"//.*", "", kernels)) == [], stage
    others = {name: squeeze(read(name)) for stage in MAP_STAGES for name in (stage + "_kernels.hip", stage + ".cpp")}
    for text, times in TABLE_TEXTS.items():
        assert header.count(squeeze(text)) == times, text
        for name, source in others.items():
            assert source.count(squeeze(text)) == (1 if (text, name) == (PROBE_LOOP, "voxel_map_kernels.hip") else 0), (text, name)
    return header


def _cells(params):
    return [max(1, int(math.ceil((params["hi"][k] - params["lo"][k]) / params["size"]))) for k in range(3)]


def row_key(params, p, pose, w):
    """(key, u) of one row p = (x, y, z) with weight w under `pose` (12 floats), or None for a dropped row."""
    if w <= 0:
        return None
    x, y, z = (float(v) for v in p)
    key, u = 0, []
    cells = _cells(params)
    for k in range(3):
        try:
            P = ((pose[3 * k] * x + pose[3 * k + 1] * y) + pose[3 * k + 2] * z) + pose[9 + k]
        except OverflowError:
            return None
        if not (params["lo"][k] < P < params["hi"][k]):
            return None
        t = (P - params["lo"][k]) / params["size"]
        c = min(int(t), cells[k] - 1)
        u.append(min(int((t - float(c)) * 65536.0), 65535))
        key |= c << (20 * k)
    return key, u


def frame_keys(params, call):
    """Per frame of a call the list of its contributed rows' keys, None for a dropped row."""
    xyz, color, n, counts, poses = call
    out = []
    for b in range(xyz.shape[0]):
        rows = []
        for i in range(max(0, min(int(counts[b]), xyz.shape[1]))):
            r = row_key(params, xyz[b, i], [float(v) for v in poses[b]], 1 if n is None else int(n[b, i]))
            rows.append(None if r is None else r[0])
        out.append(rows)
    return out


def table_updates(params, calls, combine=True):
    """The table updates the insert kernel issues: with the merge one per run of equal keys among the kept rows of a segment of 64 rows
    of a frame - a dropped row ends a run -, without it one per kept row."""
    total = 0
    for call in calls:
        for rows in frame_keys(params, call):
            for s in range(0, len(rows), 64):
                seg = rows[s:s + 64]
                for i, k in enumerate(seg):
                    if k is not None and (not combine or i + 1 == len(seg) or seg[i + 1] != k):
                        total += 1
    return total


def model_voxel_map(params, calls, min_n=1, min_rows=1, since=0, dtype="f32"):
    """voxel_map_rows' dict, with "dropped" and "claimed" besides, from a loop over the rows of all calls; the frames are numbered on
    from call to call."""
    vox, dropped, seq0, over = {}, 0, 0, False
    for xyz, color, n, counts, poses in calls:
        B, cap = xyz.shape[:2]
        for b in range(B):
            pose = [float(v) for v in poses[b]]
            for i in range(max(0, min(int(counts[b]), cap))):
                w = 1 if n is None else int(n[b, i])
                r = row_key(params, xyz[b, i], pose, w)
                if r is None:
                    dropped += 1
                    continue
                key, u = r
                v = vox.setdefault(key, {"n": 0, "S": [0, 0, 0], "C": [0, 0, 0, 0], "m": 0, "first": seq0 + b, "last": seq0 + b})
                v["n"] += w
                v["m"] += 1
                for k in range(3):
                    v["S"][k] += w * u[k]
                for j in range(4):
                    v["C"][j] += 0 if color is None else w * int(color[b, i, j])
                v["first"], v["last"] = min(v["first"], seq0 + b), max(v["last"], seq0 + b)
        seq0 += B
        over = over or len(vox) > params["capacity"]
    keys = [] if over else sorted(k for k, v in vox.items() if v["n"] >= min_n and v["m"] >= min_rows and v["last"] >= since)
    V = len(keys)
    out = {"xyz": np.zeros((V, 3), np.float64), "color": np.zeros((V, 4), np.uint8), "cell": np.zeros((V, 3), np.int32), "n": np.zeros(V, np.int64),
           "m": np.zeros(V, np.int64), "first_seq": np.zeros(V, np.int32), "last_seq": np.zeros(V, np.int32), "key": np.array(keys, np.int64).reshape(V)}
    for r, key in enumerate(keys):
        v = vox[key]
        for k in range(3):
            c = (key >> (20 * k)) & 0xFFFFF
            out["cell"][r, k] = c
            out["xyz"][r, k] = params["lo"][k] + (float(c) + (float(v["S"][k]) + 0.5 * float(v["n"])) / (65536.0 * float(v["n"]))) * params["size"]
        for j in range(4):
            out["color"][r, j] = (2 * v["C"][j] + v["n"]) // (2 * v["n"])
        out["n"][r], out["m"][r], out["first_seq"][r], out["last_seq"][r] = v["n"], v["m"], v["first"], v["last"]
    if dtype == "f32":
        out["xyz"] = out["xyz"].astype(np.float32)
    out.update(count=-1 if over else V, dropped=dropped, claimed=len(vox))
    return out


# ------------------------------------------------------------------------------------------------------------------ painted cases

def cell_points(cells, frac=0.5):
    """float64 [n,3]: a point inside each cell (cx, cy, cz) of BOX16-like unit cells at offset `frac` on every axis."""
    return np.asarray(cells, np.float64).reshape(-1, 3) + frac


def one_frame(xyz, color=None, n=None, pose=IDENTITY, dtype=np.float64, count=None):
    xyz = np.asarray(xyz, dtype)[None]
    return (xyz, None if color is None else np.asarray(color, np.uint8)[None], None if n is None else np.asarray(n, np.int32)[None],
            np.array([xyz.shape[1] if count is None else count], np.int32), np.asarray(pose, np.float64)[None])


def distinct_cells(count, side=16):
    i = np.arange(count)
    return np.stack([i % side, (i // side) % side, i // (side * side)], -1)


def painted_cases():
    """{name: (params, calls, the table updates the merge must issue)}."""
    rng = np.random.default_rng(5)
    cases = {}
    for rows in (64, 65, 257):  # a run that ends at lane 63, crosses a wavefront's edge, crosses a workgroup's edge
        pts = np.tile(cell_points([(3, 4, 5)]), (rows, 1)) + rng.uniform(-0.4, 0.4, (rows, 3))
        col = rng.integers(0, 256, (rows, 4)).astype(np.uint8)
        cases["one_voxel_%d" % rows] = (BOX16, [one_frame(pts, col)], -(-rows // 64))
    cases["every_row_its_own"] = (BOX16, [one_frame(cell_points(distinct_cells(300)), rng.integers(0, 256, (300, 4)))], 300)
    pts = np.tile(cell_points([(7, 7, 7)]), (40, 1))
    pts[17] = np.nan  # a dropped row in the middle of a run: two runs
    cases["run_cut_by_a_dropped_row"] = (BOX16, [one_frame(pts, np.full((40, 4), 9))], 2)
    big = np.tile(cell_points([(15, 15, 15)], 1.0 - 2.0 ** -20), (64, 1))  # u = 65535 on every axis
    cases["largest_payload"] = (BOX16, [one_frame(big, np.full((64, 4), 255), np.full(64, 2 ** 31 - 1))], 1)
    mixed = cell_points(np.repeat(distinct_cells(30), rng.integers(1, 9, 30), 0))  # runs of 1 .. 8 rows
    cases["short_runs"] = (BOX16, [one_frame(mixed, rng.integers(0, 256, (len(mixed), 4)), rng.integers(1, 50, len(mixed)), dtype=np.float32)], None)
    return cases


PROBE_BOX = dict(lo=(0.0, 0.0, 0.0), hi=(64.0, 64.0, 64.0), size=1.0, capacity=512)  # 64 cells per axis: enough keys to choose colliding ones


def colliding_cells(slot_of, slot, count, slots=1024):
    """`count` cells of PROBE_BOX whose keys slot_of sends to `slot`."""
    c = distinct_cells(64 ** 3, 64)
    key = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
    hit = np.flatnonzero(slot_of(key, slots) == slot)[:count]
    assert len(hit) == count
    return c[hit]


def random_case(seed):
    """A small random map of at most 8 x 8 x 4 cells and one call of 1 .. 3 frames: f32 or f64 rows, with or without colours and
    weights, rows outside the box, on cell boundaries and not finite, counts of 0, -1 and above cap."""
    rng = np.random.default_rng(1000 + seed)
    size = float(rng.choice([0.25, 0.5, 1.0, 0.3, 0.7]))
    cells = rng.integers(1, [9, 9, 5])
    lo = np.round(rng.uniform(-3, 3, 3), 1)
    hi = lo + cells * size - (size * 0.25 if seed % 3 == 0 else 0.0)  # every third map ends inside its last cell
    params = dict(lo=tuple(lo.tolist()), hi=tuple(hi.tolist()), size=size, capacity=512)
    B, cap = int(rng.integers(1, 4)), int(rng.integers(1, 200))
    xyz = lo + rng.uniform(-0.1, 1.1, (B, cap, 3)) * (hi - lo)
    snap = rng.random((B, cap)) < 0.2
    xyz[snap] = lo + np.round((xyz[snap] - lo) / size) * size  # on a cell boundary
    bad = rng.random((B, cap)) < 0.05
    xyz[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    xyz = xyz.astype(np.float32 if seed % 2 else np.float64)
    color = rng.integers(0, 256, (B, cap, 4)).astype(np.uint8) if seed % 4 < 2 else None
    n = rng.integers(-1, 40, (B, cap)).astype(np.int32) if seed % 5 < 3 else None
    counts = rng.integers(0, cap + 1, B).astype(np.int32)
    counts[rng.random(B) < 0.15] = -1
    counts[rng.random(B) < 0.15] = cap + 7
    yaw = rng.uniform(-0.2, 0.2, B) * (seed % 2)
    c, s, z = np.cos(yaw), np.sin(yaw), np.zeros(B)
    poses = np.stack([c, -s, z, s, c, z, z, z, z + 1, rng.uniform(-0.3, 0.3, B), rng.uniform(-0.3, 0.3, B), rng.uniform(-0.1, 0.1, B)], -1)
    return params, [(xyz, color, n, counts, poses)]
