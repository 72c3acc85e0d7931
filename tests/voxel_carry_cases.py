"""Inputs for a voxel map carried into another (group (S)) and an independent model of it: a Python dict of voxels and one loop per
voxel, Python ints only.  A case is a dict: dst and src, each (params, calls) as voxel_map_cases has them, and kw - shift and the filters
of voxel_map_carry."""
import numpy as np

import voxel_map_cases as cases
from voxel_map_cases import BOX16, PROBE_BOX

STATS = ("carried", "filtered", "outside", "claimed")


def model_map(params, calls):
    """{"vox": {key: voxel}, "dropped", "over", "params"} from a loop over the rows of all calls, the frames numbered on from call to call."""
    vox, dropped, seq0, over = {}, 0, 0, False
    for xyz, color, n, counts, poses in calls:
        B, cap = xyz.shape[:2]
        for b in range(B):
            pose = [float(v) for v in poses[b]]
            for i in range(max(0, min(int(counts[b]), cap))):
                w = 1 if n is None else int(n[b, i])
                r = cases.row_key(params, xyz[b, i], pose, w)
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
    return {"vox": vox, "dropped": dropped, "over": over, "params": params}


def model_carry(dst, src, shift=(0, 0, 0), min_n=1, min_rows=1, since=0):
    """The definition, voxel by voxel: dst (model_map's dict) is changed, -> the four counts."""
    stats = dict.fromkeys(STATS, 0)
    dst["dropped"] += src["dropped"]
    if src["over"] or dst["over"]:
        dst["over"] = True
        stats["carried"] = -1
        return stats
    cells = cases._cells(dst["params"])
    for key, v in src["vox"].items():
        if not (v["n"] >= min_n and v["m"] >= min_rows and v["last"] >= since):
            stats["filtered"] += 1
            continue
        c = [((key >> (20 * k)) & 0xFFFFF) + shift[k] for k in range(3)]
        if any(c[k] < 0 or c[k] > cells[k] - 1 for k in range(3)):
            stats["outside"] += 1
            continue
        stats["carried"] += 1
        moved = c[0] | c[1] << 20 | c[2] << 40
        if moved not in dst["vox"]:
            stats["claimed"] += 1
            dst["vox"][moved] = {"n": 0, "S": [0, 0, 0], "C": [0, 0, 0, 0], "m": 0, "first": v["first"], "last": v["last"]}
        d = dst["vox"][moved]
        d["n"] += v["n"]
        d["m"] += v["m"]
        d["S"] = [a + b for a, b in zip(d["S"], v["S"])]
        d["C"] = [a + b for a, b in zip(d["C"], v["C"])]
        d["first"], d["last"] = min(d["first"], v["first"]), max(d["last"], v["last"])
    if len(dst["vox"]) > dst["params"]["capacity"]:
        dst["over"] = True
    return stats


def model_rows(m):
    """voxel_map_rows' dict (dtype "f64") of a model map, with "dropped", "claimed" and "overflowed" besides."""
    params, vox = m["params"], m["vox"]
    keys = [] if m["over"] else sorted(vox)
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
    out.update(count=-1 if m["over"] else V, dropped=m["dropped"], claimed=len(vox), overflowed=m["over"])
    return out


# ------------------------------------------------------------------------------------------------------------------ cases

def frames(cells_per_frame, colors=True, weights=None, frac=0.5, seed=0):
    """One call of len(cells_per_frame) frames, frame b holding a point in each of its cells (padded with rows beyond the count)."""
    rng = np.random.default_rng(seed)
    cap = max(len(c) for c in cells_per_frame)
    B = len(cells_per_frame)
    xyz, counts = np.zeros((B, cap, 3)), np.zeros(B, np.int32)
    for b, c in enumerate(cells_per_frame):
        xyz[b, :len(c)] = cases.cell_points(c, frac) if len(c) else 0
        counts[b] = len(c)
    color = rng.integers(0, 256, (B, cap, 4)).astype(np.uint8) if colors else None
    n = None if weights is None else rng.integers(weights[0], weights[1] + 1, (B, cap)).astype(np.int32)
    return (xyz, color, n, counts, np.tile(cases.IDENTITY, (B, 1)))


def slot_cells(slot_of, wanted, slots=1024):
    """One cell of PROBE_BOX per slot of `wanted` whose key slot_of sends there: keys that never collide with each other."""
    c = cases.distinct_cells(64 ** 3, 64)
    key = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
    h = slot_of(key, slots)
    first = {}
    for i in np.flatnonzero(np.isin(h, np.asarray(wanted))):
        first.setdefault(int(h[i]), i)
    assert len(first) == len(set(int(w) for w in wanted))
    return c[[first[int(w)] for w in wanted]]


def hand_case():
    """Four voxels of src - one filtered, one shifted out, one onto a voxel of dst, one onto a free cell - with every number written out in
    test_hand_case."""
    src_cells = [[(1, 1, 1), (2, 2, 2), (15, 3, 3)], [(1, 1, 1), (4, 4, 4)], [(4, 4, 4)]]  # frames 0, 1, 2
    src = (BOX16, [(cases.cell_points(np.array(src_cells[0]), 0.25)[None], np.array([[[10, 20, 30, 40]] * 3], np.uint8), np.array([[3, 1, 2]], np.int32),
                    np.array([3], np.int32), cases.IDENTITY[None]),
                   (np.concatenate([cases.cell_points(np.array(src_cells[1]), 0.75), [[99.0, 0, 0]]])[None], np.array([[[50, 60, 70, 80]] * 3], np.uint8),
                    np.array([[5, 7, 1]], np.int32), np.array([3], np.int32), cases.IDENTITY[None]),
                   (cases.cell_points(np.array(src_cells[2]), 0.5)[None], np.array([[[0, 0, 0, 255]]], np.uint8), np.array([[1]], np.int32),
                    np.array([1], np.int32), cases.IDENTITY[None])])
    dst = (BOX16, [(cases.cell_points(np.array([(0, 0, 0)]), 0.5)[None], None, None, np.array([1], np.int32), cases.IDENTITY[None]),
                   (cases.cell_points(np.array([(2, 2, 2), (9, 9, 9)]), 0.5)[None], np.array([[[100, 100, 100, 100]] * 2], np.uint8), np.array([[4, 6]], np.int32),
                    np.array([2], np.int32), cases.IDENTITY[None])])
    return dict(dst=dst, src=src, kw=dict(shift=(1, 1, 1), min_n=2))


def carry_cases(slot_of):
    """{name: case}, shared by the CPU tests (the numpy form against the model) and the GPU tests (the device against the numpy form)."""
    rng = np.random.default_rng(11)
    out = {"hand": hand_case()}
    empty16 = (BOX16, [])
    # the filters one below, at and one above each threshold: voxels of n = 4, 5, 6; of m = 1, 2, 3; of last_seq = 0, 1, 2
    rows = [[(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 0, 0), (2, 0, 0), (1, 0, 0)], [(4, 0, 0), (5, 0, 0)], [(5, 0, 0), (6, 0, 0)]]
    n = np.ones((3, 6), np.int32)
    n[0] = [4, 2, 2, 2, 2, 3]
    thresholds = (BOX16, [(frames(rows)[0], frames(rows)[1], n, frames(rows)[3], frames(rows)[4])])
    for name, kw in (("min_n", "min_n"), ("min_rows", "min_rows"), ("since", "since")):
        for v in ((4, 5, 6, 7) if kw == "min_n" else (0, 1, 2, 3)):
            out["filter_%s_%d" % (name, v)] = dict(dst=empty16, src=thresholds, kw={kw: v})
    out["filters_together"] = dict(dst=empty16, src=thresholds, kw=dict(min_n=2, min_rows=2, since=0))
    # c + shift at -1, 0, cells - 1 and cells on each axis: cells 0, 1, 14, 15 of an axis under shifts of -1, 0 and +1
    edge = [(a, b, c) for a in (0, 1, 14, 15) for b in (0, 15) for c in (0, 15)] + [(7, a, 7) for a in (1, 14)] + [(7, 7, a) for a in (1, 14)]
    edges = (BOX16, [frames([edge], seed=1)])
    for shift in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1), (1, -1, 1), (-15, 15, 0), (16, 0, 0), (0, 0, -16)):
        out["shift_%d_%d_%d" % shift] = dict(dst=empty16, src=edges, kw=dict(shift=shift))
    narrow = (dict(BOX16, hi=(16.0, 3.0, 1.0)), [])  # a destination of 16 x 3 x 1 cells: its own cells decide, not the source's
    out["shift_into_a_smaller_box"] = dict(dst=narrow, src=edges, kw=dict(shift=(0, 1, 0)))
    # a merge: keys that coincide and keys that do not; first_seq / last_seq win from either side
    a = [[(1, 1, 1), (2, 2, 2)], [], [], [(3, 3, 3)], [(1, 1, 1)]]           # dst: frames 0 .. 4
    b = [[(2, 2, 2)], [(3, 3, 3), (5, 5, 5)], [(1, 1, 1)], [], [], [], [(3, 3, 3)]]  # src: frames 0 .. 6
    out["merge"] = dict(dst=(BOX16, [frames(a, weights=(1, 9), seed=2)]), src=(BOX16, [frames(b, weights=(1, 9), frac=0.25, seed=3)]), kw={})
    out["merge_shifted_filtered"] = dict(dst=(BOX16, [frames(a, seed=2)]), src=(BOX16, [frames(b, seed=3)]), kw=dict(shift=(-1, -1, -1), since=2))
    out["colours_into_none"] = dict(dst=(BOX16, [frames(a, colors=False, seed=2)]), src=(BOX16, [frames(b, seed=3)]), kw={})
    out["none_into_colours"] = dict(dst=(BOX16, [frames(a, seed=2)]), src=(BOX16, [frames(b, colors=False, seed=3)]), kw={})
    # dropped rows are carried over
    lost = frames([[(1, 1, 1), (40, 0, 0), (2, 2, 2), (0, -3, 0)]], seed=4)
    out["dropped"] = dict(dst=(BOX16, [frames([[(1, 1, 1), (0, 99, 0)]], seed=5)]), src=(BOX16, [lost]), kw={})
    # an overflowed source, and an overflowed destination
    three = frames([[(1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 77, 0)]], seed=6)
    out["overflowed_source"] = dict(dst=(BOX16, [frames(a, seed=2)]), src=(dict(BOX16, capacity=2), [three]), kw={})
    out["overflowed_destination"] = dict(dst=(dict(BOX16, capacity=2), [three]), src=(BOX16, [frames(a, seed=2)]), kw={})
    # the destination at its capacity exactly, and one above: 512 keys no two of which collide in a table of 1024 slots
    free = slot_cells(slot_of, range(0, 1024, 2))
    full = (PROBE_BOX, [frames([free[:300], free[300:]], seed=7)])
    out["capacity_exactly"] = dict(dst=(PROBE_BOX, []), src=full, kw={})
    out["capacity_one_above"] = dict(dst=(dict(PROBE_BOX, capacity=511), []), src=full, kw={})
    out["capacity_one_above_merge"] = dict(dst=(dict(PROBE_BOX, capacity=300), [frames([free[:100]], seed=8)]), src=(PROBE_BOX, [frames([free[99:301]], seed=9)]), kw={})
    # zero shift, no filter, an empty destination: the source again
    some = cases.distinct_cells(16 ** 3)[rng.permutation(16 ** 3)[:400]]
    cloud = (BOX16, [frames([some[:250], some[150:]], weights=(1, 1000), seed=10)])
    out["copy"] = dict(dst=empty16, src=cloud, kw={})
    return out


def gpu_cases(slot_of):
    """More cases for the device: where its probing, its tiles and its 64-bit words turn over."""
    out = {}
    # keys that all start probing at one slot, at the last slots of the destination's table: chains that wrap from slot 1023 to 0
    for slot in (1020, 1023):
        chain = cases.colliding_cells(slot_of, slot, 12)
        out["probe_wrap_%d" % slot] = dict(dst=(PROBE_BOX, [frames([chain[:5]], seed=20)]), src=(PROBE_BOX, [frames([chain[3:]], seed=21)]), kw={})
        out["probe_wrap_empty_%d" % slot] = dict(dst=(PROBE_BOX, []), src=(PROBE_BOX, [frames([chain], seed=22)]), kw={})
    # a source tile whose 256 slots are all occupied, and a single voxel in lane 63 of a wavefront
    tile = slot_cells(slot_of, range(256, 512))
    out["full_tile"] = dict(dst=(PROBE_BOX, []), src=(PROBE_BOX, [frames([tile], seed=23)]), kw={})
    out["full_tile_merge"] = dict(dst=(PROBE_BOX, [frames([tile[::3]], seed=24)]), src=(PROBE_BOX, [frames([tile], seed=23)]), kw={})
    out["lane_63"] = dict(dst=(PROBE_BOX, []), src=(PROBE_BOX, [frames([slot_cells(slot_of, [767])], seed=25)]), kw={})
    # n past 2^32 and S past 2^48: 512 rows of weight 2^31 - 1 at offset 65535 in one cell, then added to themselves
    big = np.tile(cases.cell_points([(15, 15, 15)], 1.0 - 2.0 ** -20), (512, 1))
    heavy = (BOX16, [cases.one_frame(big, np.full((512, 4), 255), np.full(512, 2 ** 31 - 1))])
    out["wide_words"] = dict(dst=(BOX16, []), src=heavy, kw={})
    out["wide_words_merge"] = dict(dst=heavy, src=heavy, kw={})
    # a destination larger and smaller than the source: 1024 slots against 8192
    rng = np.random.default_rng(12)
    some = cases.distinct_cells(64 ** 3, 64)[rng.permutation(64 ** 3)[:500]]
    cloud = frames([some[:300], some[200:]], weights=(1, 50), seed=26)
    out["grow"] = dict(dst=(dict(PROBE_BOX, capacity=4096), []), src=(PROBE_BOX, [cloud]), kw={})
    out["shrink"] = dict(dst=(PROBE_BOX, []), src=(dict(PROBE_BOX, capacity=4096), [cloud]), kw=dict(min_rows=2))
    return out
