"""Inputs for the carve of the voxel map (group (T)) and an independent model of it: one Python loop per ray, Python ints and floats only.
A case is a dict: params (lo, hi, size, capacity), calls (the inserts that build the map, as voxel_map_cases' - the frames are numbered on
from call to call), frames = (xyz, n, counts, poses) as voxel_map_carve takes them, and kw (origin, seq0, reach, margin, min_miss, ratio).
Unless a case says otherwise the box is BOX16 - 16 x 16 x 16 cells of size 1, capacity 512 - and the pose the identity, so that a point
(cx + 0.5, cy + 0.5, cz + 0.5) lies in cell (cx, cy, cz) and `origin` names the sensor's cell the same way."""
import math

import numpy as np

import voxel_map_cases as cases
from voxel_map_cases import BOX16, IDENTITY, PROBE_BOX, cell_points, one_frame

STATS = ("rays", "steps", "touched", "carved")
CENTRE = (8.5, 8.5, 8.5)  # the sensor in cell (8, 8, 8)


def key_of(c):
    return int(c[0]) | int(c[1]) << 20 | int(c[2]) << 40


def cell_of(key):
    return (key & 0xFFFFF, (key >> 20) & 0xFFFFF, (key >> 40) & 0xFFFFF)


def ray_cells(c0, c1, margin):
    """The cells of the steps k = 1 .. nst - 1 - margin of the ray from cell c0 to cell c1, and nst: Python's flooring division."""
    d = [c1[a] - c0[a] for a in range(3)]
    nst = max(abs(v) for v in d)
    return [tuple(c0[a] + (2 * k * d[a] + nst) // (2 * nst) for a in range(3)) for k in range(1, nst - margin)], nst


def model_carve(params, voxels, frames, origin=(0.0, 0.0, 0.0), seq0=0, reach=1023, margin=1, min_miss=1, ratio=0):
    """voxels: {key: (n, last_seq)} of the map, a tombstone as (0, 0).  -> (stats dict, {key: miss} of the touched voxels, the set of the
    carved keys).  One ray at a time."""
    xyz, n, counts, poses = frames
    stats, miss = dict.fromkeys(STATS, 0), {}
    for b in range(xyz.shape[0]):
        pose = [float(v) for v in poses[b]]
        if not all(math.isfinite(v) for v in pose):
            continue
        sensor = cases.row_key(params, origin, pose, 1)
        if sensor is None:
            continue
        c0 = cell_of(sensor[0])
        for i in range(max(0, min(int(counts[b]), xyz.shape[1]))):
            w = 1 if n is None else int(n[b, i])
            row = cases.row_key(params, xyz[b, i], pose, w)
            if row is None:
                continue
            cells, nst = ray_cells(c0, cell_of(row[0]), margin)
            if nst > reach:
                continue
            stats["rays"] += 1
            stats["steps"] += len(cells)
            assert len(set(cells)) == len(cells)  # a ray visits no cell twice
            for c in cells:
                v = voxels.get(key_of(c))
                if v is not None and v[1] < seq0 + b:
                    miss[key_of(c)] = miss.get(key_of(c), 0) + w
    carved = {k for k, m in miss.items() if m >= min_miss and 256 * m >= ratio * voxels[k][0]}
    stats["touched"], stats["carved"] = len(miss), len(carved)
    return stats, miss, carved


def voxels_of(state):
    """{key: (n, last_seq)} of a numpy map state, for model_carve; an emptied voxel reads as last_seq 0."""
    return {int(k): (int(n), max(int(last), 0)) for k, n, last in zip(state["key"], state["n"], state["last_seq"])}


def frames_of(points, n=None, pose=IDENTITY, dtype=np.float64, count=None):
    """One frame of rows at `points` as voxel_map_carve takes it."""
    xyz, _, n, counts, poses = one_frame(points, None, n, pose, dtype, count)
    return xyz, n, counts, poses


def stack_frames(*frames):
    """Frames of one row count each, as one batch; weights where any frame has them."""
    cap = max(f[0].shape[1] for f in frames)
    dtype = frames[0][0].dtype
    xyz = np.full((len(frames), cap, 3), np.nan, dtype)
    n = np.ones((len(frames), cap), np.int32) if any(f[1] is not None for f in frames) else None
    for b, f in enumerate(frames):
        xyz[b, :f[0].shape[1]] = f[0][0]
        if f[1] is not None:
            n[b, :f[1].shape[1]] = f[1][0]
    return xyz, n, np.concatenate([f[2] for f in frames]).astype(np.int32), np.concatenate([f[3] for f in frames])


def _case(calls, frames, params=BOX16, **kw):
    return dict(params=params, calls=calls, frames=frames, kw=kw)


def hand_case():
    """Sensor in cell (2, 2, 2); voxels A = (4, 2, 2) with n 1 and B = (6, 2, 2) with n 4 on the ray to (8, 2, 2), C = (6, 3, 2) off it.  One row
    of weight 3, margin 1: the steps visit x = 3, 4, 5, 6.  A and B get miss 3; with min_miss 3 and ratio 256, A (256 * 3 >= 256 * 1) is
    carved and B (768 < 1024) is not."""
    calls = [one_frame(cell_points([(4, 2, 2), (6, 2, 2), (6, 3, 2)]), None, [1, 4, 2])]
    return _case(calls, frames_of(cell_points([(8, 2, 2)]), [3]), origin=(2.5, 2.5, 2.5), seq0=1, reach=16, margin=1, min_miss=3, ratio=256)


def cube_surface(half):
    g = np.arange(-half, half + 1)
    d = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return d[np.abs(d).max(1) == half]


def direction_case():
    """From the centre cell to every cell on the surface of a 9^3 cube - all sign combinations, all three major axes -, and rays of six
    steps whose minor axes move by -3: every odd step lies half way.  The map holds the 7^3 cells inside the cube."""
    inner = np.stack(np.meshgrid(*[np.arange(5, 12)] * 3, indexing="ij"), -1).reshape(-1, 3)
    ends = np.concatenate([8 + cube_surface(4), [(14, 5, 8), (2, 11, 5), (5, 2, 11), (11, 5, 14), (5, 14, 5)]])
    return _case([one_frame(cell_points(inner))], frames_of(cell_points(ends)), origin=CENTRE, seq0=1, reach=8, margin=0)


def rounding_census(case):
    """(steps of a minor axis with d < 0 whose 2 k d + nst is an exact multiple of 2 nst, steps whose flooring and truncating quotients
    differ) over the rays of a one-frame case under the identity."""
    c0 = tuple(int(v) for v in case["kw"]["origin"])
    exact = differ = 0
    for p in case["frames"][0][0]:
        d = [int(p[a]) - c0[a] for a in range(3)]
        nst = max(abs(v) for v in d)
        for k in range(1, nst - case["kw"]["margin"]):
            for a in range(3):
                num = 2 * k * d[a] + nst
                exact += d[a] < 0 and abs(d[a]) < nst and num % (2 * nst) == 0
                differ += num // (2 * nst) != int(num / (2 * nst))
    return exact, differ


X_LINE = [(x, 8, 8) for x in range(3, 9)]  # voxels on the +x axis from the sensor cell (2, 8, 8)


def limit_cases():
    """nst == reach and reach + 1 (one row each), nst == 0, and every margin around nst = 5."""
    calls = [one_frame(cell_points(X_LINE))]
    rows = cell_points([(7, 8, 8), (8, 8, 8), (2, 8, 8), (2, 3, 8), (2, 8, 14)])  # nst = 5, 6, 0, 5, 6
    return {"limits_margin_%d" % m: _case(calls, frames_of(rows), origin=(2.5, 8.5, 8.5), seq0=1, reach=5, margin=m) for m in (0, 1, 3, 4, 7, 255)}


def long_axis_cases():
    """1100 cells along x, and along z: rays of nst = 1023 in the negative direction - 1022 steps -, keys up to c << 40 and step terms up
    to 2 * 1022 * 1023 + 1023."""
    out = {}
    for axis in (0, 2):
        hi = [2.0, 2.0, 2.0]
        hi[axis] = 1100.0
        params = dict(lo=(0.0, 0.0, 0.0), hi=tuple(hi), size=1.0, capacity=512)

        def at(long, u, v, axis=axis):
            c = [u, v]
            c.insert(axis, long)
            return tuple(c)

        # from (1090, 1, 1) to (67, 0, 0): the minor axes step down behind k = 511
        held = [at(1000, 1, 1), at(600, 1, 1), at(600, 0, 0), at(490, 0, 0), at(490, 1, 1), at(68, 0, 0), at(579, 1, 0), at(578, 1, 0), at(578, 0, 1), at(1089, 1, 1), at(30, 0, 0)]
        ends = [at(67, 0, 0), at(67, 1, 1), at(67, 0, 1), at(68, 1, 0), at(66, 0, 0)]  # the last is 1024 away: no ray
        origin = tuple(v + 0.5 for v in at(1090, 1, 1))
        out["long_axis_%s" % "xyz"[axis]] = _case([one_frame(cell_points(held))], frames_of(cell_points(ends), [1, 2, 4, 8, 16]), params, origin=origin, seq0=1,
                                                  reach=1023, margin=0)
    return out


def sequence_cases():
    """Voxels last seen at 0, 1 and 2 under a frame numbered 1; and a batch of two frames carved with the batch that inserted it: frame 1
    counts against what only frame 0 saw, frame 0 does not."""
    three = [one_frame(cell_points([(5, 8, 8)])), one_frame(cell_points([(6, 8, 8)])), one_frame(cell_points([(7, 8, 8)]))]
    guard = _case(three, frames_of(cell_points([(10, 8, 8)])), origin=(2.5, 8.5, 8.5), seq0=1, reach=16, margin=0)
    f0, f1 = frames_of(cell_points([(5, 8, 8), (10, 8, 8)])), frames_of(cell_points([(10, 8, 8), (10, 8, 9)]))
    batch = stack_frames(f0, f1)
    insert = (batch[0], None, batch[1], batch[2], batch[3])
    return {"sequence_guard": guard, "sequence_batch": _case([insert], batch, origin=(2.5, 8.5, 8.5), seq0=0, reach=16, margin=0)}


def _random_map(rng, count=300):
    c = rng.integers(0, 16, (count, 3))
    return [one_frame(cell_points(c), None, rng.integers(1, 9, count))]


def layout_cases():
    rng = np.random.default_rng(11)
    out = {}
    # 64 lanes of one wavefront through one voxel
    out["one_wavefront_one_voxel"] = _case([one_frame(cell_points([(5, 8, 8)]))], frames_of(np.tile(cell_points([(9, 8, 8)]), (64, 1)), np.arange(1, 65)),
                                           origin=(2.5, 8.5, 8.5), seq0=1, reach=16, margin=1, min_miss=64 * 65 // 2)
    # 513 and 257 rows - rays that straddle wavefronts and workgroups -, counts below cap with NaN and huge values beyond, a frame that
    # casts nothing in the middle
    cap = 513
    xyz = rng.uniform(0.0, 16.0, (3, cap, 3))
    xyz[1, 257:] = np.where(rng.random((cap - 257, 3)) < 0.5, np.nan, 1e300)
    poses = np.tile(IDENTITY, (3, 1))
    poses[1, 9:] = (0.25, -0.25, 0.125)
    poses[2, 4] = np.nan
    frames = (xyz, rng.integers(1, 5, (3, cap)).astype(np.int32), np.array([513, 257, 400], np.int32), poses)
    out["straddling_rows"] = _case(_random_map(rng), frames, origin=(8.25, 7.75, 8.5), seq0=1, reach=16, margin=1, min_miss=6, ratio=300)
    with np.errstate(over="ignore"):  # 1e300 is inf as a float
        narrow = xyz[[2, 0, 1]].astype(np.float32)
    swapped = (narrow, None, np.array([400, 513, 257], np.int32), poses[[2, 0, 1]])
    out["straddling_rows_f32"] = _case(_random_map(rng), swapped, origin=(8.25, 7.75, 8.5), seq0=1, reach=9, margin=0, min_miss=2)
    out["counts_zero_and_negative"] = _case(_random_map(rng), (xyz[:2, :40], None, np.array([0, -5], np.int32), poses[:2]), origin=CENTRE, seq0=1, reach=16)
    return out


def caster_cases():
    rng = np.random.default_rng(12)
    rows = rng.uniform(0.0, 16.0, (120, 3))
    n = rng.integers(-2, 6, 120).astype(np.int32)  # weights <= 0 are dropped
    rows[::7] = rng.uniform(-3.0, 19.0, (len(rows[::7]), 3))  # outside
    rows[3::11, 1] = np.nan
    rows[5::13, 0] = np.inf
    calls = _random_map(rng)
    out = {}
    for name, origin, pose in (("sensor_on_a_face", (0.0, 8.5, 8.5), IDENTITY), ("sensor_on_the_far_face", (8.5, 16.0, 8.5), IDENTITY),
                               ("sensor_outside", (8.5, 8.5, -0.5), IDENTITY), ("sensor_inside", CENTRE, IDENTITY),
                               ("pose_not_finite", CENTRE, np.where(np.arange(12) == 2, np.inf, IDENTITY)),
                               ("quarter_turn", (8.5, 7.5, 8.5), cases.QUARTER + np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 16.0, 0.0, 0.0]))):
        for dtype in (np.float64, np.float32):
            turned = rows if name != "quarter_turn" else np.stack([rows[:, 1], 16.0 - rows[:, 0], rows[:, 2]], -1)
            out["%s_%s" % (name, np.dtype(dtype).name)] = _case(calls, frames_of(turned, n, pose, dtype), origin=origin, seq0=1, reach=12, margin=1, min_miss=3)
    return out


def wide_cases():
    big = 2 ** 31 - 1
    out = {"miss_above_2_32": _case([one_frame(cell_points([(5, 8, 8)]), None, [big])], frames_of(np.tile(cell_points([(9, 8, 8)]), (5, 1)), [big] * 5),
                                    origin=(2.5, 8.5, 8.5), seq0=1, reach=16, margin=1, min_miss=5 * big, ratio=5 * 256)}
    held = [one_frame(cell_points([(5, 8, 8), (6, 8, 8)]), None, [12, 12])]  # two voxels of weight 12
    through = lambda w: frames_of(cell_points([(9, 8, 8), (9, 8, 8), (5, 8, 8)]), [3, w, 1])  # noqa: E731 - the third row ends in the first voxel: no step there
    out["ratio_exact"] = _case(held, through(3), origin=(2.5, 8.5, 8.5), seq0=1, reach=16, margin=1, min_miss=1, ratio=128)        # 256 * 6 == 128 * 12
    out["ratio_one_below"] = _case(held, through(2), origin=(2.5, 8.5, 8.5), seq0=1, reach=16, margin=1, min_miss=1, ratio=128)    # 256 * 5 < 128 * 12
    out["min_miss_at"] = _case(held, through(3), origin=(2.5, 8.5, 8.5), seq0=1, reach=16, margin=1, min_miss=6, ratio=0)
    out["min_miss_above"] = _case(held, through(3), origin=(2.5, 8.5, 8.5), seq0=1, reach=16, margin=1, min_miss=7, ratio=0)
    return out


def chain_case(slot_of, slot=77):
    """A, B, C: three cells of PROBE_BOX whose keys start probing at one slot, inserted in that order - the chain A, B, C -, and a ray of
    three steps along an axis through B alone."""
    a, b, c = (tuple(int(v) for v in cell) for cell in cases.colliding_cells(slot_of, slot, 3))
    axis = next(k for k in range(3) if 2 <= b[k] <= 61)
    step = np.eye(3, dtype=np.int64)[axis]
    start, end = tuple(np.array(b) - 2 * step), tuple(np.array(b) + 2 * step)
    on_ray = ray_cells(start, end, 0)[0]
    assert b in on_ray and a not in on_ray and c not in on_ray and len(on_ray) == 3
    calls = [one_frame(cell_points([cell]), None, [5]) for cell in (a, b, c)]
    case = _case(calls, frames_of(cell_points([end]), [2]), PROBE_BOX, origin=tuple(float(v) + 0.5 for v in start), seq0=3, reach=8, margin=0)
    return case, (a, b, c)


def all_cases(slot_of):
    out = {"hand": hand_case(), "directions": direction_case(), "probe_chain": chain_case(slot_of)[0]}
    for more in (limit_cases(), long_axis_cases(), sequence_cases(), layout_cases(), caster_cases(), wide_cases()):
        assert not set(more) & set(out)
        out.update(more)
    return out


def overflowed_case():
    return _case([one_frame(cell_points(cases.distinct_cells(3)))], frames_of(cell_points([(9, 8, 8)])), dict(BOX16, capacity=2), origin=CENTRE, seq0=1, reach=16)
