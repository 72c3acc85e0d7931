"""Inputs for the voxel map flattened into an occupancy map (group (V)).  A case is a dict: params and calls as voxel_map_cases has them
(one call per update), flat (the flat map's nine words), spec (the seven words of the height rule) and kw (min_n, min_rows, since).  Every
voxel map holds at most 2048 voxels in a table of 1024 to 4096 slots and every flat map at most 65 x 70 cells, and each case is there
because one mistake shows on it."""
import numpy as np

from voxel_map_cases import BOX16, IDENTITY, cell_points, one_frame

WIDE = dict(lo=(-8.0, -8.0, -1.0), hi=(72.0, 72.0, 7.0), size=0.5, capacity=2048)  # 160 x 160 x 16 cells, a table of 4096 slots
TALL = dict(lo=(0.0, 0.0, 0.0), hi=(16.0, 16.0, 80.0), size=1.0, capacity=512)     # 80 cells of height: a column of 64 and more voxels
LOG_ODDS = dict(l_occ=85, l_free=40, l_min=-200, l_max=350)
SHAPES = {"1x1": ((3, 4), (5, 6)), "7x31": ((0, 7), (0, 31)), "8x32": ((0, 8), (0, 32)), "9x33": ((0, 9), (0, 33)), "64x64": ((0, 64), (0, 64)),
          "65x70": ((-1, 64), (-2, 68)), "negative": ((-7, -2), (-6, -1))}  # x_range, y_range at one cell per metre; the last has top = -2 and left = -1


def flat_words(x_range, y_range, scale, **log_odds):
    """occupancy_map_params' dict, written out."""
    w = dict(top=x_range[1] * scale, left=y_range[1] * scale, rows=(x_range[1] - x_range[0]) * scale, cols=(y_range[1] - y_range[0]) * scale, scale=scale)
    return dict(w, **dict(LOG_ODDS, **log_odds))


def words(mode=1, z_ref_q=0, step_q=102, height_q=1024, radius=2, min_obstacle=1, min_ground=1):
    """The height rule's words; the defaults are 0.2 m and 2 m at a voxel of 0.5 m."""
    return dict(mode=mode, z_ref_q=z_ref_q, step_q=step_q, height_q=height_q, radius=radius, min_obstacle=min_obstacle, min_ground=min_ground)


def case(params, calls, flat, spec, **kw):
    return dict(params=params, calls=calls, flat=flat, spec=spec, kw=kw)


def at_zq(x, y, zq, size=1.0, lo_z=0.0):
    """A point in the column (x, y) whose voxel, of this one row, has the height zq: cell zq // 256 and offset (zq % 256) << 8, plus half
    an offset unit so that no rounding moves it."""
    return [x, y, lo_z + (zq // 256 + (((zq % 256) << 8) + 0.5) / 65536.0) * size]


def crowd(x_range, y_range, count, seed, margin=2.0):
    """`count` weighted rows over the ranges and a margin around them: a floor up to 0.3 m, every fifth row an obstacle up to 1.8 m, every
    seventh overhead at 3 to 5 m."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform([x_range[0] - margin, y_range[0] - margin, 0.0], [x_range[1] + margin, y_range[1] + margin, 0.3], (count, 3))
    pts[::5, 2] = rng.uniform(0.5, 1.8, len(pts[::5]))
    pts[::7, 2] = rng.uniform(3.0, 5.0, len(pts[::7]))
    return one_frame(pts, None, rng.integers(1, 9, count))


def shape_cases():
    """Every flat shape at which a tile of the clear, floor (16 x 64 cells) or resolve kernel turns over, under a local floor."""
    out = {}
    for k, (name, (xr, yr)) in enumerate(SHAPES.items()):
        calls = [crowd(xr, yr, min(1800, max(200, 40 + 2 * (xr[1] - xr[0]) * (yr[1] - yr[0]))), 20 + k)]
        out["shape_" + name] = case(WIDE, calls, flat_words(xr, yr, 1), words(radius=2))
    xr, yr = SHAPES["65x70"]
    out["shape_65x70_radius8"] = case(WIDE, [crowd(xr, yr, 1800, 31)], flat_words(xr, yr, 1), words(radius=8))
    out["shape_65x70_absolute"] = case(WIDE, [crowd(xr, yr, 1800, 32)], flat_words(xr, yr, 1), words(mode=0, z_ref_q=512))  # lo_z = -1 m: z = 0 is zq 512
    return out


def incommensurate_cases():
    """Voxel sizes that no flat cell is a multiple of: 0.3 m at two cells per metre, 0.5 m at four."""
    out = {}
    for name, size, scale in (("size03_scale2", 0.3, 2), ("size05_scale4", 0.5, 4)):
        params = dict(lo=(-3.1, -2.9, -0.7), hi=(-3.1 + 64 * size, -2.9 + 64 * size, -0.7 + 16 * size), size=size, capacity=2048)
        calls = [crowd((0, 12), (0, 14), 1500, 40 + scale, margin=1.0)]
        out["incommensurate_" + name] = case(params, calls, flat_words((0, 12), (0, 14), scale), words(step_q=int(round(0.2 / size * 256)), height_q=int(round(2.0 / size * 256))))
    return out


def border_case():
    """Voxels of two rows of weight 1 each, at the offsets (0, 65535) of one axis: (S + 0.5 n) / (65536 n) = 65536 / 131072 = 0.5 exactly,
    so at two flat cells per voxel cell X ms is a whole number: the centre lies on a flat cell's border and floor() must put it above.
    Their neighbours, at (0, 65534) and (1, 65535), miss the border by 1 / 131072 of a cell on either side."""
    def pair(cell, axis, u0, u1):
        p = cell_points([cell, cell])
        p[0, axis], p[1, axis] = cell[axis] + (u0 + 0.5) / 65536.0, cell[axis] + (u1 + 0.5) / 65536.0
        return p
    pts = np.concatenate([pair((2 + 2 * k, 3, 0), 0, u0, u1) for k, (u0, u1) in enumerate(((0, 65535), (0, 65534), (1, 65535)))]
                         + [pair((3, 2 + 2 * k, 0), 1, u0, u1) for k, (u0, u1) in enumerate(((0, 65535), (0, 65534), (1, 65535)))])
    return case(BOX16, [one_frame(pts)], flat_words((0, 16), (0, 16), 2), words(step_q=51, height_q=512))


def contention_case():
    """One flat cell that holds a column of 70 voxels - one ground, seven obstacles up to 8 m, 62 overhead - while its eight neighbours hold
    one each: every atomic of both walks meets its rivals there."""
    column = [(5, 5, z) for z in range(70)]
    ring = [(5 + dx, 5 + dy, 0) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy) != (0, 0)]
    return case(TALL, [one_frame(cell_points(column + ring))], flat_words((0, 16), (0, 16), 1), words(step_q=256, height_q=8 * 256, radius=1))


def outside_cases():
    calls = [crowd((0, 16), (0, 16), 600, 50, margin=-0.5)]
    return {"outside_four_sides": case(BOX16, calls, flat_words((5, 9), (6, 11), 1), words(step_q=51, height_q=512)),
            "outside_wholly": case(BOX16, calls, flat_words((100, 104), (0, 16), 1), words(step_q=51, height_q=512))}


THRESHOLD = dict(z_ref_q=1000, step_q=50, height_q=400)
THRESHOLD_ZQ = [1000 + t + d for t in (-50, 50, 400) for d in (-1, 0, 1)]  # below | ground, ground | obstacle, obstacle | overhead


def threshold_case():
    """Mode 0: a voxel one zq unit below, at and above each of -step_q, step_q and height_q over the floor, each in a flat cell of its own."""
    pts = [at_zq(1.5 + k, 2.5, zq) for k, zq in enumerate(THRESHOLD_ZQ)]
    return case(BOX16, [one_frame(pts)], flat_words((0, 16), (0, 16), 1), words(mode=0, **THRESHOLD))


RING_AT = (20, 20)  # the lone low voxel of ring_cases, as (x, y) cells of WIDE-like unit cells


def ring_cases():
    """Mode 1 on a 64 x 64 map: a lone low voxel A whose floor reaches 8 cells and no further; B, 8 cells away on the diagonal, and D, 9
    cells away, hold one voxel 1.5 cells up each - an obstacle over A's floor, ground over its own -; a wall column W whose lowest voxel
    lies 3 cells up beside a ground voxel G; and a voxel in each corner and on each edge, whose windows the map clips.  Run at radius 0,
    1 and 8."""
    params = dict(lo=(0.0, 0.0, 0.0), hi=(64.0, 64.0, 16.0), size=1.0, capacity=512)
    ax, ay = RING_AT
    pts = [at_zq(ax + 0.5, ay + 0.5, 10), at_zq(ax + 8.5, ay + 8.5, 384), at_zq(ax + 9.5, ay + 0.5, 384)]
    pts += [at_zq(40.5, 40.5, 20), at_zq(41.5, 40.5, 768), at_zq(41.5, 40.5, 1024), at_zq(41.5, 40.5, 1280)]  # G, then W
    pts += [at_zq(x + 0.5, y + 0.5, 300 + 7 * k) for k, (x, y) in enumerate(((0, 0), (0, 63), (63, 0), (63, 63), (0, 30), (63, 30), (30, 0), (30, 63)))]
    pts += [at_zq(x + 0.5, y + 0.5, 700) for x, y in ((1, 1), (1, 62), (62, 1), (62, 62), (1, 30), (62, 30), (30, 1), (30, 62))]  # obstacles over them from radius 1 on
    calls = [one_frame(pts)]
    out = {"ring_radius%d" % r: case(params, calls, flat_words((0, 64), (0, 64), 1), words(step_q=128, height_q=2048, radius=r)) for r in (0, 1, 8)}
    out["ring_small_map"] = case(params, calls, flat_words((38, 43), (39, 42), 1), words(step_q=128, height_q=2048, radius=8))  # 5 x 3 cells under a window of 17 x 17
    return out


COUNTED = dict(ground=2, obstacle=3)  # of the cell of counted_cases


def counted_cases():
    """A cell with two ground and three obstacle voxels, with min_obstacle and min_ground one below, at and one above its counts."""
    pts = [at_zq(4.5, 4.5, zq) for zq in (0, 300, 600, 900, 1200)]  # step_q 512: the first two are ground
    calls = [one_frame(pts)]
    flat = flat_words((0, 16), (0, 16), 1)
    out = {}
    for mo in (2, 3, 4):
        for mg in (1, 2, 3):
            out["counted_o%d_g%d" % (mo, mg)] = case(BOX16, calls, flat, words(mode=0, step_q=512, height_q=4096, min_obstacle=mo, min_ground=mg))
    return out


CLAMPED = dict(column=(6, 34, 30), ground=6)  # clamp_cases: the column's ground, obstacle and overhead voxels, and the second cell's ground voxels


def clamp_cases():
    """The products obstacle * l_occ and ground * l_free above the clamps, above 32767 before them, and below them: a column of 70 voxels
    (34 obstacles) and a cell of six ground voxels."""
    calls = [one_frame(cell_points([(5, 5, z) for z in range(70)] + [(9, 9, z) for z in range(6)]))]
    spec = words(mode=0, step_q=6 * 256, height_q=40 * 256)
    return {"clamp_default": case(TALL, calls, flat_words((0, 16), (0, 16), 1), spec),
            "clamp_wide": case(TALL, calls, flat_words((0, 16), (0, 16), 1, l_occ=32767, l_free=32767, l_min=-32767, l_max=32767), spec),
            "clamp_not_reached": case(TALL, calls, flat_words((0, 16), (0, 16), 1, l_occ=900, l_free=5000, l_min=-32767, l_max=32767), spec)}


def filter_cases():
    """One flat cell, four voxels at four heights: X1 n = 2, m = 2, last 1; X2 n = 5, m = 1, last 1; X3 n = 5, m = 2, last 0; X4 n = 5, m =
    2, last 1.  Each filter drops another of the first three, and with it the cell's low, its top or a count."""
    col = lambda z: [4.5, 4.5, z + 0.5]  # noqa: E731
    rows0 = (np.array([col(2), col(2), [0, 0, 0], [0, 0, 0], [0, 0, 0]], np.float64), np.array([2, 3, 0, 0, 0], np.int32))
    rows1 = (np.array([col(0), col(0), col(1), col(3), col(3)], np.float64), np.array([1, 1, 5, 2, 3], np.int32))
    xyz, n = np.stack([rows0[0], rows1[0]]), np.stack([rows0[1], rows1[1]])
    calls = [(xyz, None, n, np.array([2, 5], np.int32), np.stack([IDENTITY, IDENTITY]))]
    flat = flat_words((0, 16), (0, 16), 1)
    return {"filter_" + name: case(BOX16, calls, flat, words(step_q=300, height_q=700, radius=0), **kw)
            for name, kw in (("none", {}), ("min_n", dict(min_n=3)), ("min_rows", dict(min_rows=2)), ("since", dict(since=1)))}


def overflowed_cases():
    calls = [one_frame(cell_points([(4, 4, 4), (5, 4, 4)]))]
    flat = flat_words((0, 9), (0, 33), 1)
    return {"overflowed_local": case(dict(BOX16, capacity=1), calls, flat, words(radius=2)),
            "overflowed_absolute": case(dict(BOX16, capacity=1), calls, flat, words(mode=0, z_ref_q=-77))}


def empty_case():
    return case(BOX16, [], flat_words((0, 9), (0, 33), 1), words(radius=8))


# ------------------------------------------------------------------------------------------------------------------ the planner's scene

SCENE_BOX = dict(lo=(0.0, 0.0, -0.5), hi=(16.0, 16.0, 7.5), size=0.5, capacity=2048)
SCENE_FLAT = ((0, 16), (0, 16), 1)
SCENE_START, SCENE_GOAL = (1.5, 2.5), (14.5, 2.5)
SCENE_WALL_X, SCENE_WALL_Y = 8, 12     # the wall fills the flat cells x = 8, y < 12: the way round it is y >= 12
SCENE_SLAB_X = (3, 6)                  # the slab hangs over x in 3 .. 6, every y, 3 m above the floor


def scene_points():
    """float64 [n,3]: a flat floor of 16 x 16 m at z = 0.1, a wall one flat cell thick from the floor to 2 m, and a slab 3 m above the floor
    from one side of the map to the other: whoever drives from SCENE_START to SCENE_GOAL passes under the slab and round the wall."""
    g = np.arange(0.25, 16.0, 0.5)
    floor = np.stack(np.meshgrid(g, g, [0.1], indexing="ij"), -1).reshape(-1, 3)
    wall = np.stack(np.meshgrid([8.25, 8.75], g[g < SCENE_WALL_Y], [0.6, 1.1, 1.6], indexing="ij"), -1).reshape(-1, 3)
    slab = np.stack(np.meshgrid(g[(g > SCENE_SLAB_X[0]) & (g < SCENE_SLAB_X[1])], g, [3.1], indexing="ij"), -1).reshape(-1, 3)
    return np.concatenate([floor, wall, slab])


def scene_case():
    return case(SCENE_BOX, [one_frame(scene_points())], flat_words(*SCENE_FLAT), words())


def all_cases():
    """{name: case}."""
    cases = {"border": border_case(), "contention": contention_case(), "threshold": threshold_case(), "empty": empty_case(), "scene": scene_case()}
    for more in (shape_cases(), incommensurate_cases(), outside_cases(), ring_cases(), counted_cases(), clamp_cases(), filter_cases(), overflowed_cases()):
        cases.update(more)
    return cases
