"""Inputs for the voxel map rendered into a camera (group (U)).  A case is a dict: params and calls as voxel_map_cases has them (one call
per update), cams float64 [V,12] (world to camera), camera (the dict voxel_render_camera makes, written out), measured (float32 [V,H,W] or
None) and kw (near, far, r_max, tol, min_n, min_rows, since).  Every map holds at most a few hundred voxels and every image is at most
70 x 9, and each case is there because one mistake shows on it."""
import numpy as np

from voxel_map_cases import BOX16, IDENTITY, PROBE_BOX, cell_points, colliding_cells, one_frame

HALF = 4.0 + 32768.5 / 65536.0  # the centre, on an axis, of a voxel of one row at cell_points' frac 0.5 in cell 4: exact in double
VIEWS = 8                       # the views a workgroup of the table walks draws into (csrc/voxel_render_kernels.h: VRENDER_VIEWS)


def camera(width=16, height=9, f=8.0, cx=0.0, cy=0.0, half_px=0.0, q32=2.0, q33=0.25):
    return dict(f=f, cx=cx, cy=cy, q32=q32, q33=q33, half_px=half_px, width=width, height=height)


def moved(tx=0.0, ty=0.0, tz=0.0):
    """The camera with the world's axes, its centre at (-tx, -ty, -tz)."""
    p = IDENTITY.copy()
    p[9:] = tx, ty, tz
    return p


def aimed(at, u, v, cam, depth=None):
    """The camera with the world's axes under which the world point `at` lands at (u, v) of `cam`, at its own depth or at `depth`."""
    z = at[2] if depth is None else depth
    return moved((u - cam["cx"]) * z / cam["f"] - at[0], (v - cam["cy"]) * z / cam["f"] - at[1], z - at[2])


def key_of(cell):
    return int(cell[0]) | int(cell[1]) << 20 | int(cell[2]) << 40


def case(params, calls, cams, cam, measured=None, **kw):
    return dict(params=params, calls=calls, cams=np.asarray(cams, np.float64).reshape(-1, 12), camera=cam, measured=measured, kw=kw)


def colors(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, (n, 4)).astype(np.uint8)


def hand_case():
    """Two voxels on pixel (5, 5) - (1.5, 1.5, 2.5) and, twice as far on the same ray, (3, 3, 5), both plus 1 / 131072 - and one alone on
    pixel (1, 1)."""
    pts = np.concatenate([cell_points([(1, 1, 2)]), cell_points([(3, 3, 5)], 0.0), cell_points([(0, 0, 4)])])
    col = np.array([[10, 20, 30, 40], [50, 60, 70, 80], [90, 100, 110, 120]], np.uint8)
    return case(BOX16, [one_frame(pts, col)], [IDENTITY], camera(8, 7, q33=0.0))


def depth_order_case(slot_of):
    """Pairs of voxels on one ray each: in one the nearer voxel lies at the lower slot of the table, in the other at the higher."""
    found = {}
    for i in range(4):
        for j in range(3):
            near, far = (i, j, 2), (2 * i + 1, 2 * j + 1, 5)
            lower = int(slot_of(key_of(near), 1024)) < int(slot_of(key_of(far), 1024))
            found.setdefault(lower, (near, far))
    assert len(found) == 2
    pts = np.concatenate([np.concatenate([cell_points([near]), cell_points([far], 0.0)]) for near, far in found.values()])
    return case(BOX16, [one_frame(pts, colors(4))], [IDENTITY], camera())


def equal_depth_pair(slot_of):
    """Two cells of one z plane of PROBE_BOX whose keys start at the same slot, at most 30 cells apart - neighbours never collide under
    a multiplicative hash -, so far away that they project within 5 pixels of each other: with r = 4 their squares overlap."""
    for z in range(50, 60):
        c = np.stack(np.meshgrid(np.arange(64), np.arange(64), [z], indexing="ij"), -1).reshape(-1, 3)
        slot = slot_of(c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40), 1024)
        for a in range(len(c)):
            near = np.flatnonzero((slot == slot[a]) & (np.abs(c - c[a]).max(1) <= 30) & (np.abs(c - c[a]).max(1) > 0))
            if len(near):
                return c[a], c[near[0]]
    raise AssertionError("no colliding pair")


def equal_depth_cases(slot_of):
    """The same two voxels - equal zq, overlapping squares, colliding keys - inserted in either order: the slots swap, the render does not."""
    a, b = equal_depth_pair(slot_of)
    pa, pb = cell_points([a])[0], cell_points([b])[0]
    cam = camera(20, 9, half_px=4.5 * (a[2] + 1.0))
    pose = aimed((pa + pb) / 2, 9.7, 4.2, cam)
    frames = [one_frame([p], [col]) for p, col in ((pa, (1, 2, 3, 4)), (pb, (5, 6, 7, 8)))]
    return {"equal_depth_ab": case(PROBE_BOX, frames, [pose], cam, r_max=4), "equal_depth_ba": case(PROBE_BOX, frames[::-1], [pose], cam, r_max=4)}


def footprint_cases():
    one = [one_frame(cell_points([(4, 4, 4)]), [(9, 8, 7, 6)])]  # its centre: (HALF, HALF, HALF), tz = HALF
    at = (HALF, HALF, HALF)
    out = {}
    for name, half_px, r_max in (("r0", 0.0, 4), ("r_at_r_max", 2 * HALF, 2), ("r_capped", 3 * HALF + 0.1, 2), ("r_below_integer", 2 * HALF * (1 - 2.0 ** -40), 4),
                                 ("r_at_integer", 2 * HALF, 4), ("r_largest", 9 * HALF, 8)):
        cam = camera(half_px=half_px)
        out["footprint_" + name] = case(BOX16, one, [aimed(at, 8.2, 4.2, cam)], cam, r_max=r_max)
    cam = camera(12, 8, half_px=2 * HALF)  # r = 2
    spots = [(0.2, 3.2), (11.2, 3.2), (5.2, 0.2), (5.2, 7.2), (0.2, 0.2), (11.2, 7.2),  # clipped at each border, and at two corners
             (-1.8, 3.2), (13.2, 9.2),  # centres outside whose squares reach in
             (-2.8, 3.2), (5.2, 10.2), (14.2, 3.2), (5.2, -2.8)]  # squares that miss by one pixel: not drawn
    out["footprint_borders"] = case(BOX16, one, [aimed(at, u, v, cam) for u, v in spots], cam, r_max=2)
    return out


def depth_range_cases():
    pts = np.concatenate([cell_points([(4, 4, 4)]), cell_points([(6, 4, 7)])])
    calls = [one_frame(pts, colors(2))]
    cam = camera()
    views = [IDENTITY, moved(0, 0, -10.0), moved(0, 0, -HALF), moved(0, 0, 1e300), moved(np.nan, 0, 0)]  # as it is; behind; Pc[2] == 0 for the first; far away; NaN
    return {"depth_near_kept": case(BOX16, calls, views, cam, near=HALF, far=7.6),
            "depth_far_dropped": case(BOX16, calls, views, cam, near=1.0, far=HALF),
            "depth_open": case(BOX16, calls, views, cam)}


def filter_cases():
    """X1 n = 2, m = 2, last 1; X2 n = 5, m = 1, last 1; X3 n = 5, m = 2, last 0; X4 n = 5, m = 2, last 1: each filter drops one of the first three."""
    x1, x2, x3, x4 = (1, 1, 4), (3, 1, 4), (5, 1, 4), (7, 1, 4)
    rows0 = (np.concatenate([cell_points([x3, x3]), np.zeros((3, 3))]), np.array([2, 3, 0, 0, 0], np.int32))
    rows1 = (cell_points([x1, x1, x2, x4, x4]), np.array([1, 1, 5, 2, 3], np.int32))
    xyz, n = np.stack([rows0[0], rows1[0]]), np.stack([rows0[1], rows1[1]])
    calls = [(xyz, np.stack([colors(5, 2), colors(5, 3)]), n, np.array([2, 5], np.int32), np.stack([IDENTITY, IDENTITY]))]
    cam = camera(half_px=HALF)
    return {"filter_" + name: case(BOX16, calls, [IDENTITY], cam, **kw)
            for name, kw in (("none", {}), ("min_n", dict(min_n=3)), ("min_rows", dict(min_rows=2)), ("since", dict(since=1)))}


def table_case(slot_of):
    """Three voxels whose probe chain starts in the table's last slot and wraps to its first, each looked at by a view of its own."""
    cells = colliding_cells(slot_of, 1023, 3)
    pts = cell_points(cells)
    cam = camera(half_px=5.0)
    return case(PROBE_BOX, [one_frame(pts, colors(3, 4))], [aimed(p, 3.2 + k, 3.2, cam, depth=5.0) for k, p in enumerate(pts)], cam)


def crowd(count, seed):
    """`count` rows in the lower half of BOX16, with colours and weights: a few share a cell."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(0.5, 15.5, (count, 3)) * [1, 1, 0.5]
    return one_frame(pts, colors(count, seed), rng.integers(1, 9, count))


def view_cases():
    """V = 0, 1 and around the view group's size, every view with a pose of its own, into 70 x 5 and 1 x 1 images."""
    rng = np.random.default_rng(7)
    calls = [crowd(150, 8)]
    out = {}
    for V in (0, 1, VIEWS - 1, VIEWS, VIEWS + 1):
        yaw = rng.uniform(-0.3, 0.3, V)
        c, s, z = np.cos(yaw), np.sin(yaw), np.zeros(V)
        cams = np.stack([c, z, -s, z, z + 1, z, s, z, c, rng.uniform(-9, -7, V), rng.uniform(-9, -7, V), rng.uniform(2, 6, V)], -1)  # a turn about y
        out["views_%d" % V] = case(BOX16, calls, cams, camera(70, 5, f=30.0, cx=35.0, cy=2.0, half_px=20.0))
        out["views_%d_one_pixel" % V] = case(BOX16, calls, cams, camera(1, 1, f=1.0, half_px=8.0), r_max=8)
    return out


def comparison_case(sv):
    """A measured map painted over the render of a crowd so that every label occurs: valid and not - NaN, inf, 0, negative - on pixels
    with and without a winner; on winners d = e's float32 (agree), |d - e| exactly at tol (agree), one float further (not), far nearer and
    far farther."""
    calls = [crowd(120, 9)]
    cam = camera(40, 9, f=20.0, cx=20.0, cy=4.0, half_px=12.0)
    cams = np.stack([moved(-8.0, -8.0, 3.0), moved(-7.5, -7.8, 4.0)])
    state = sv.voxel_map_state(sv.voxel_map_params(**BOX16))
    sv.voxel_map_insert(state, *calls[0])
    seen = sv.voxel_map_render(state, cams, cam)
    has, e32 = seen["depth"] >= 0, seen["disparity"]
    assert has.sum() > 60 and (~has).sum() > 60
    z = ((seen["depth"].astype(np.float64) + 0.5) / 256.0) * 1.0
    e = (cam["f"] / z - cam["q33"]) / cam["q32"]
    rng = np.random.default_rng(10)
    measured = np.where(has, e32, np.float32(3.0)).astype(np.float32)
    pick = rng.integers(0, 9, has.shape)
    for k, value in ((0, np.nan), (1, 0.0), (2, -2.0), (3, np.inf)):
        measured[pick == k] = value
    measured[has & (pick == 4)] += np.float32(0.75)   # d - e is about 0.75: the tolerance below is one such difference, exactly
    measured[has & (pick == 5)] += np.float32(5.0)    # nearer
    measured[has & (pick == 6)] = np.float32(0.001)   # farther
    at = np.argwhere(has & (pick == 4))[0]
    tol = float(np.float64(measured[tuple(at)]) - e[tuple(at)])  # the pixel `at` sits exactly at tol
    assert tol > 0.5
    return case(BOX16, calls, cams, cam, measured=measured, tol=tol)


def overflowed_case():
    return case(dict(BOX16, capacity=1), [one_frame(cell_points([(4, 4, 4), (5, 4, 4)]))], [IDENTITY, IDENTITY], camera(),
                measured=np.array([[[1.0, np.nan]]], np.float32).repeat(2, 0).repeat(9, 1).repeat(8, 2))


def empty_case():
    return case(BOX16, [], [IDENTITY, moved(1.0, 0, 0)], camera(), measured=np.array([[[2.0, -1.0]]], np.float32).repeat(2, 0).repeat(9, 1).repeat(8, 2))


def all_cases(sv):
    """{name: case}."""
    slot_of = sv.voxel_map_slot_of
    cases = {"hand": hand_case(), "depth_order": depth_order_case(slot_of), "table_wrap": table_case(slot_of), "comparison": comparison_case(sv),
             "overflowed": overflowed_case(), "empty": empty_case()}
    for more in (equal_depth_cases(slot_of), footprint_cases(), depth_range_cases(), filter_cases(), view_cases()):
        cases.update(more)
    return cases
