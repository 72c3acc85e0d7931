"""Occupancy and elevation grids (include/stereo_vision_hip.h (J)): the numpy definition in stereo_vision.sv on a hand-built map, the
sight lines' closed form and its clip on random cell pairs, a synthetic scene with a known wall, the argument checks in Python and in
the C ABI, and the HIP kernels - C entry, engine, rig and CLI - against the definition.

Everything is compared exactly.  That is derived, not chosen: the point of a pixel is reproject.h's arithmetic in double without FMA on
both sides, and everything behind trunc() - the cell, the height step, the counts, the minimum and maximum, the sight lines' cells and
the state - is integer work whose result does not depend on any order."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)

SV_ERR_ARG = -1
NAN, INF = float("nan"), float("inf")
W, H = 1242, 375
OUTPUTS = ("cells", "n_rays", "state")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- CPU

# 4 rows x 6 columns.  With HAND_Q a pixel (u, v) of disparity d lies at X = 8 / d, Y = (2 - u) / d, Z = (1 - v) / d: everything below
# is exact.  The grid is x 0..8, y -2..2, z -1..1 at scale 1: 9 x 5 cells, cell (8 - trunc(X), 2 - trunc(Y)), the origin in cell (8, 2).
# z_scale = 65536: h = min(trunc((Z + 1) * 65536), 65535).
HAND_Q = np.array([[0, 0, 0, 8.0], [-1, 0, 0, 2.0], [0, -1, 0, 1.0], [0, 0, 1, 0]])
HAND_GRID = dict(x_range=(0, 8), y_range=(-2, 2), z_range=(-1, 1), scale=1, z_scale=65536)
HAND_D = np.array([[-10, 4, -10, -10, -10, -10],   # (1, 0) obstacle: X 2, Y 0.25, Z 0.25 -> cell (6, 2), h = 81920 -> 65535
                   [1, 4, -10, -10, -10, -10],     # (0, 1) obstacle: X = 8, on the bound: dropped; (1, 1) obstacle: cell (6, 2), Z 0 -> 65536 -> 65535
                   [-10, -10, 2, 2, -10, 2],       # (2, 2), (3, 2) ground: X 4, Y 0 / -0.5, Z -0.5 -> cell (4, 2), h = 32768; (5, 2) label 3
                   [-10, -10, 2, -10, 4, 4]], np.float32)  # (2, 3) ground: Z = -1, on the bound: dropped; (4, 3) ground: X 2, Y -0.5, Z -0.5 ->
#                                                            cell (6, 2), h = 32768; (5, 3) label 0 under a valid disparity
HAND_LABELS = np.array([[0, 2, 0, 0, 0, 0],
                        [2, 2, 0, 0, 0, 1],        # (5, 1): label 1 over an invalid disparity - no ground pixel, so column 5 casts no line
                        [0, 0, 1, 1, 0, 3],
                        [0, 0, 1, 0, 1, 0]], np.uint8)
# column 0: an obstacle end at X 16, Y 4 -> cell (-8, -2) outside the grid: n = 16, steps 0..8 are inside; column 1: an obstacle end in
# cell (6, 2): steps 0, 1; columns 2 and 3: ground ends (2, 2) and (3, 2), both in cell (4, 2): steps 0..4; column 4: an obstacle end at
# X 0.5, Y -0.125 - the origin's own cell, n = 0: nothing; column 5: no line
HAND_FREE_ROW = np.array([1, 1, -1, -1, 3, -1], np.int32)
HAND_FREE_DISP = np.array([0.5, 4, 0, 0, 16, 0], np.float32)
HAND_CELLS = {(4, 2): (2, 0, 32768, 32768), (6, 2): (1, 2, 32768, 65535)}
HAND_RAYS = {(8, 2): 4, (7, 2): 4, (6, 2): 3, (5, 2): 2, (4, 2): 2, (5, 1): 1, (4, 1): 1, (3, 1): 1, (2, 1): 1, (1, 0): 1, (0, 0): 1}


def _hand(sv, **kw):
    return sv.occupancy_grid(HAND_D, HAND_LABELS, HAND_FREE_ROW, HAND_FREE_DISP, HAND_Q, **dict(HAND_GRID, **kw))


def test_hand_built_map(sv):
    want_cells = np.zeros((9, 5, 4), np.int32)
    want_cells[..., 2:] = -1
    for rc, t in HAND_CELLS.items():
        want_cells[rc] = t
    want_rays = np.zeros((9, 5), np.int32)
    for rc, n in HAND_RAYS.items():
        want_rays[rc] = n
    got = _hand(sv, min_obstacle=2)
    assert got["cells"].dtype == np.int32 and got["n_rays"].dtype == np.int32 and got["state"].dtype == np.uint8
    assert np.array_equal(got["cells"], want_cells) and np.array_equal(got["n_rays"], want_rays)
    want_state = np.where(want_rays > 0, 1, 0).astype(np.uint8)
    want_state[6, 2] = 2
    assert np.array_equal(got["state"], want_state)
    # the defaults: two obstacle pixels are fewer than min_obstacle = 3, the cell's ground pixel makes it free
    dflt = _hand(sv)
    assert dflt["state"][6, 2] == 1 and np.array_equal(dflt["cells"], want_cells)
    # thresholds: no ray count reaches 5, cell (4, 2) holds two ground pixels and cell (6, 2) one
    hard = _hand(sv, min_obstacle=3, min_ground=2, min_rays=5)
    assert hard["state"][4, 2] == 1 and hard["state"].sum() == 1
    assert np.array_equal(_hand(sv, min_obstacle=3, min_ground=3, min_rays=4)["state"] == 1, want_rays >= 4)
    # the heights in metres: step 32768 of 65536 above z0 = -1, NaN where empty
    z_lo, z_hi = sv.occupancy_heights(got["cells"], -1, 65536)
    assert z_lo[4, 2] == -0.5 and z_hi[4, 2] == -0.5 and z_lo[6, 2] == -0.5 and z_hi[6, 2] == -1 + 65535 / 65536
    assert np.isnan(z_lo).sum() == 43 and np.isnan(z_hi).sum() == 43
    # a coarser height step: Z = -0.5, 0, 0.25 -> trunc(0.5 * 3), trunc(1 * 3), trunc(1.25 * 3)
    assert _hand(sv, z_scale=3)["cells"][6, 2].tolist() == [1, 2, 1, 3]
    # an origin outside the grid: XT = (0, 3, 0) puts the camera centre in cell (8, -1) and every pixel's point at Y >= 2.5, out of
    # range.  Only column 3's line reaches the grid: its ground end (X 4, Y 2.5) lies in cell (4, 0), dr = -4, dc = 1, n = 4, and
    # c_k = -1 + (2 k + 4) // 8 is 0 from k = 2 on.  Column 0 runs to cell (-8, -5), columns 1 and 2 end in column -1, column 4 has
    # n = 1 and leaves out its end, the only cell of its line inside
    moved = _hand(sv, XT=(0, 3, 0))
    want_moved = np.zeros((9, 5), np.int32)
    want_moved[[6, 5, 4], 0] = 1
    assert moved["cells"][..., :2].sum() == 0 and np.array_equal(moved["n_rays"], want_moved) and np.array_equal(moved["state"], want_moved)
    # no ground: every valid pixel is 3, no free-space row - everything unknown
    none = sv.occupancy_grid(HAND_D, np.where(HAND_D > 0, 3, 0).astype(np.uint8), np.full(6, -1, np.int32), np.zeros(6, np.float32), HAND_Q, **HAND_GRID)
    assert not none["state"].any() and not none["n_rays"].any() and (none["cells"] == [0, 0, -1, -1]).all()


def _full_walk(r0, c0, r1, c1, obstacle):
    """The formula as the header states it, one k after the other in Python integers."""
    dr, dc = r1 - r0, c1 - c0
    n = max(abs(dr), abs(dc))
    if n == 0:
        return [] if obstacle else [(r0, c0)]
    return [(r0 + (2 * k * dr + n) // (2 * n), c0 + (2 * k * dc + n) // (2 * n)) for k in range(n if obstacle else n + 1)]


def test_ray_formula_and_clip(sv):
    rng = np.random.default_rng(71)
    octants = set()
    for trial in range(3000):
        span = int(rng.choice([3, 40, 700]))
        r0, c0, r1, c1 = (int(v) for v in rng.integers(-span, span + 1, 4))
        if trial % 5 == 0:
            r1 = r0 + int(rng.integers(-span, span + 1)) * int(rng.integers(0, 2))  # axis-parallel, diagonal and n = 0 lines too
            c1 = c0 + (r1 - r0) * int(rng.integers(-1, 2))
        dr, dc = r1 - r0, c1 - c0
        n = max(abs(dr), abs(dc))
        if dr and dc and abs(dr) != abs(dc):
            octants.add((dr > 0, dc > 0, abs(dr) > abs(dc)))
        cells = _full_walk(r0, c0, r1, c1, False)
        assert cells[0] == (r0, c0) and cells[-1] == (r1, c1) and len(cells) == n + 1
        step = np.diff(np.array(cells), axis=0)
        assert (np.abs(step) <= 1).all()
        if n:
            major = step[:, 0] if abs(dr) >= abs(dc) else step[:, 1]
            assert (major == (np.sign(dr) if abs(dr) >= abs(dc) else np.sign(dc))).all()
        for obstacle in (False, True):
            want = _full_walk(r0, c0, r1, c1, obstacle)
            assert want == cells[:len(cells) - 1] if obstacle else want == cells
            r, c = sv.occupancy_ray_cells(r0, c0, r1, c1, obstacle)
            assert list(zip(r.tolist(), c.tolist())) == want
            rows, cols = int(rng.integers(1, 60)), int(rng.integers(1, 60))
            k_lo, k_hi = sv.occupancy_ray_clip(r0, c0, r1, c1, rows, cols, obstacle)
            inside = [k for k, (a, b) in enumerate(want) if 0 <= a < rows and 0 <= b < cols]
            assert list(range(k_lo, k_hi + 1)) == inside, (r0, c0, r1, c1, rows, cols, obstacle)
            assert k_hi - k_lo + 1 <= max(rows, cols) + 1
            r, c = sv.occupancy_ray_cells(r0, c0, r1, c1, obstacle, k_lo, k_hi)
            assert list(zip(r.tolist(), c.tolist())) == [want[k] for k in inside]
    assert len(octants) == 8
    # far ends, as the kernel meets them: cells near +-2^24 around a grid at the origin
    for r1, c1 in ((2 ** 24 - 1, -(2 ** 24) + 1), (-(2 ** 24) + 1, 5), (7, 2 ** 24 - 1), (-(2 ** 24) + 1, -(2 ** 24) + 1)):
        for r0, c0 in ((3, 4), (-50, 20), (2 ** 24 - 1, 0)):
            k_lo, k_hi = sv.occupancy_ray_clip(r0, c0, r1, c1, 30, 40, True)
            r, c = sv.occupancy_ray_cells(r0, c0, r1, c1, True, k_lo, k_hi)
            assert ((r >= 0) & (r < 30) & (c >= 0) & (c < 40)).all()
            for k in (k_lo - 1, k_hi + 1):  # the neighbours of the clipped range are outside
                if 0 <= k < max(abs(r1 - r0), abs(c1 - c0)) and k_lo <= k_hi:
                    a, b = sv.occupancy_ray_cells(r0, c0, r1, c1, True, k, k)
                    assert not (0 <= a[0] < 30 and 0 <= b[0] < 40)


# a level camera 1.65 m over the ground, KITTI's focal length and baseline
F, CX, CY, BASE = 721.5377, 609.5593, 172.854, 0.54
SCENE_Q = np.array([[1, 0, 0, -CX], [0, 1, 0, -CY], [0, 0, 0, F], [0, 0, 1 / BASE, 0]])
SCENE_GRID = dict(x_range=(0, 40), y_range=(-20, 20), z_range=(-2.5, 1.5), scale=10)
WALL_D, WALL_COLS, WALL_TOP = 20.0, (500, 700), 100


def _scene():
    """Flat ground d(v) = 264 (v - 172) / (4 * 202) below the horizon row 172 - (vh, qb) = (172, 264), a camera 0.54 / 0.3267 = 1.65 m
    over it - and a fronto-parallel wall of disparity 20 (X = f b / 20 = 19.48 m) in columns 500 .. 699 from row 100 down to the row
    where the ground comes nearer than the wall; everything else invalid."""
    v = np.arange(H, dtype=np.float64)[:, None]
    d = np.where(v > 172, 264.0 * (v - 172) / (4 * 202.0), -10.0) * np.ones((1, W))
    wall = np.zeros((H, W), bool)
    wall[WALL_TOP:, WALL_COLS[0]:WALL_COLS[1]] = True
    wall &= d < WALL_D
    return np.where(wall, WALL_D, d).astype(np.float32), wall


def test_synthetic_wall(sv):
    """sv.ground fits (172, 266) to the scene, one search step from the generating (172, 264).  Recorded on the CPU, from the numpy
    definition alone: of the wall's 54 true cells (row 400 - trunc(194.8) = 206, one per grid column the wall's image columns fall into)
    54 come out occupied, a share of 1.0 (the bar is 0.9); of the 10 422 cells of the wall's grid columns between the origin and one cell
    short of the wall none is occupied (851 stay unknown, the rest is free); and of the 15 095 cells of its shadow - on the sight lines of
    the wall's inner image columns, from 0.2 m behind it to the far edge - none is free."""
    d, wall = _scene()
    g = sv.ground(d, 127)
    assert g["ground"][0] == 172 and abs(int(g["ground"][1]) - 264) <= 2  # within one search step of the generating line
    assert (g["free_row"][WALL_COLS[0]:WALL_COLS[1]] >= 0).all() and (g["labels"][wall] == 2).mean() > 0.9  # its lowest rows are within g_tol of the ground
    got = sv.occupancy_grid(d, g["labels"], g["free_row"], g["free_disp"], SCENE_Q, XR=sv.CAMERA_TO_VEHICLE, **SCENE_GRID)
    state = got["state"]
    X = F * BASE / WALL_D
    u = np.arange(*WALL_COLS, dtype=np.float64)
    row = 400 - int(np.trunc(X * 10))
    cols = np.unique(200 - np.trunc(-(u - CX) * X / F * 10).astype(np.int64))
    share = float((state[row, cols] == 2).mean())
    before = state[row + 2:, cols.min():cols.max() + 1]
    print("wall: row %d, %d cells, share occupied %.4f; before it: %d occupied, %d unknown of %d" % (row, cols.size, share, (before == 2).sum(), (before == 0).sum(), before.size))
    assert row == 206 and share >= 0.9
    assert not (before == 2).any()
    inner = u[10:-10]
    shadow = set()
    for x in np.arange(X + 0.2, 40.0, 0.05):
        r = 400 - int(np.trunc(x * 10))
        shadow |= {(r, int(c)) for c in 200 - np.trunc(-(inner - CX) * x / F * 10).astype(np.int64)}
    rr, cc = np.array(sorted(shadow)).T
    print("shadow: %d cells, %d free, %d occupied" % (len(shadow), (state[rr, cc] == 1).sum(), (state[rr, cc] == 2).sum()))
    assert len(shadow) > 3000 and not (state[rr, cc] == 1).any()
    # the ground in front of the wall is seen: free, with its height 1.65 m under the camera
    z_lo, z_hi = sv.occupancy_heights(got["cells"], SCENE_GRID["z_range"][0], 20)
    near = (slice(row + 20, row + 120), slice(cols.min(), cols.max() + 1))
    assert (state[near] == 1).all() and (got["cells"][near][..., 0] == 0).any()  # free also where no image row fell into the cell: the sight lines
    assert np.nanmax(np.abs(z_lo[near] + 1.65)) <= 0.05 + 1e-9 and np.nanmax(np.abs(z_hi[near] + 1.65)) <= 0.05 + 1e-9


_BAD_GRIDS = [dict(x_range=(0.5, 4)), dict(x_range=(4, 4)), dict(y_range=(2, -2)), dict(z_range=(1, 1)), dict(z_range=(NAN, 1)), dict(x_range=(0, INF)),
              dict(scale=0), dict(scale=-2), dict(scale=1.5), dict(x_range=(0, 40000)), dict(x_range=(0, 400), scale=100)]
_BAD_WORDS = [dict(z_scale=0), dict(z_scale=65537), dict(z_scale=-20), dict(z_scale=2.5), dict(z_scale=True), dict(min_obstacle=0), dict(min_ground=0),
              dict(min_rays=0), dict(min_rays=-1), dict(min_obstacle=2 ** 31), dict(min_ground=1.5), dict(XT=(2.0 ** 24, 0, 0)), dict(XT=(0, -2.0 ** 24, 0)),
              dict(XT=(NAN, 0, 0)), dict(XT=(0, INF, 0))]


def _c_spec(eng, reserved=None, **kw):
    p = dict(x_range=(0, 8), y_range=(-2, 2), z_range=(-1, 1), scale=1, z_scale=20, min_obstacle=3, min_ground=1, min_rays=1)
    p.update(kw)
    sp = eng.SvOccupancySpec()
    sp.x_range[:], sp.y_range[:], sp.z_range[:] = [float(v) for v in p["x_range"]], [float(v) for v in p["y_range"]], [float(v) for v in p["z_range"]]
    for k in ("scale", "z_scale", "min_obstacle", "min_ground", "min_rays"):
        setattr(sp, k, int(p[k]))
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


def test_validation_needs_no_device(sv, eng):
    """Every refused argument raises ValueError in Python; the C entry returns SV_ERR_ARG on host buffers, which stay untouched: the
    checks run before any HIP call."""
    good = dict(HAND_GRID, z_scale=20)
    for bad in _BAD_GRIDS + _BAD_WORDS:
        with pytest.raises(ValueError):
            _hand(sv, **dict(good, **bad))
        with pytest.raises(ValueError):
            eng.occupancy_spec(**{k: v for k, v in dict(good, **bad).items()})
    assert sv.occupancy_params((0, 40), (-20, 20), (-1.4, 1.0), 10)[:2] == (401, 401)
    assert sv.occupancy_params((0, 8), (-2, 2), (-INF, INF), 1, XT=(2.0 ** 24 - 1, 0.5 - 2.0 ** 24, NAN))[2] == dict(z_scale=20, min_obstacle=3, min_ground=1, min_rays=1)
    for bad in (dict(disp=HAND_D[0]), dict(labels=HAND_LABELS[:3]), dict(free_row=HAND_FREE_ROW[:5]), dict(free_disp=HAND_FREE_DISP[None])):
        a = dict(dict(disp=HAND_D, labels=HAND_LABELS, free_row=HAND_FREE_ROW, free_disp=HAND_FREE_DISP), **bad)
        with pytest.raises(ValueError):
            sv.occupancy_grid(a["disp"], a["labels"], a["free_row"], a["free_disp"], HAND_Q, **HAND_GRID)
    with pytest.raises(ValueError):
        sv.occupancy_heights(np.zeros((3, 3)), 0, 20)
    with pytest.raises(ValueError):
        sv.occupancy_heights(np.zeros((3, 4)), 0, 0)

    L = eng.occupancy_lib()
    r, c = ctypes.c_int(-7), ctypes.c_int(-7)
    bad_specs = [_c_spec(eng, reserved=k) for k in range(5)]
    bad_specs += [_c_spec(eng, **kw) for kw in _BAD_GRIDS if kw.get("scale") != 1.5]
    bad_specs += [_c_spec(eng, **kw) for kw in (dict(z_scale=0), dict(z_scale=65537), dict(z_scale=-20), dict(min_obstacle=0), dict(min_ground=0), dict(min_rays=0), dict(min_rays=-1))]
    for sp in bad_specs:
        assert L.sv_occupancy_dims(ctypes.byref(sp), ctypes.byref(r), ctypes.byref(c)) == SV_ERR_ARG and L.sv_last_error(None).startswith(b"sv_occupancy")
    assert L.sv_occupancy_dims(None, ctypes.byref(r), ctypes.byref(c)) == SV_ERR_ARG and L.sv_occupancy_dims(ctypes.byref(_c_spec(eng)), None, ctypes.byref(c)) == SV_ERR_ARG
    assert (r.value, c.value) == (-7, -7)
    assert L.sv_occupancy_dims(ctypes.byref(_c_spec(eng)), ctypes.byref(r), ctypes.byref(c)) == 0 and (r.value, c.value) == (9, 5)
    sp, rows, cols = eng.occupancy_spec((0, 40), (-20, 20), (-1.4, 1.0), 10, z_scale=65536, min_obstacle=2 ** 31 - 1)
    assert (rows, cols) == (401, 401) and L.sv_occupancy_dims(ctypes.byref(sp), ctypes.byref(r), ctypes.byref(c)) == 0 and (r.value, c.value) == (401, 401)
    assert [sp.scale, sp.z_scale, sp.min_obstacle, sp.min_ground, sp.min_rays] == [10, 65536, 2 ** 31 - 1, 1, 1] and list(sp.reserved) == [0] * 5 and ctypes.sizeof(sp) == 88

    bufs = {k: np.full(16384, 0x5A, np.uint8) for k in ("disp", "labels", "free_row", "free_disp", "cells", "n_rays", "state")}
    ptr = lambda name: bufs[name].ctypes.data  # noqa: E731
    Q, XR = np.ascontiguousarray(HAND_Q).reshape(16), np.ascontiguousarray(sv.CAMERA_TO_VEHICLE).reshape(9)
    xt = lambda *v: np.array(v, np.float64)  # noqa: E731
    keep = [xt(2.0 ** 24, 0, 0), xt(0, -2.0 ** 24, 0), xt(NAN, 0, 0), xt(0, INF, 0), xt(1, 2, 3)]
    base = dict(disp=ptr("disp"), labels=ptr("labels"), free_row=ptr("free_row"), free_disp=ptr("free_disp"), batch=2, width=16, height=8, Q=Q.ctypes.data,
                XR=XR.ctypes.data, XT=keep[4].ctypes.data, spec=_c_spec(eng), cells=ptr("cells"), n_rays=ptr("n_rays"), state=ptr("state"))
    assert ptr("cells") % 16 == 0

    def call(**kw):
        a = dict(base, **kw)
        spp = ctypes.byref(a["spec"]) if a["spec"] is not None else None
        return L.sv_occupancy_disparity_device(a["disp"], a["labels"], a["free_row"], a["free_disp"], a["batch"], a["width"], a["height"], a["Q"], a["XR"], a["XT"], spp,
                                               a["cells"], a["n_rays"], a["state"], None)

    cases = [dict(spec=None), dict(disp=None), dict(labels=None), dict(free_row=None), dict(free_disp=None), dict(Q=None), dict(cells=None), dict(n_rays=None),
             dict(batch=-1), dict(batch=65536), dict(width=0), dict(height=0), dict(width=-5), dict(width=65536, height=32768), dict(height=32769),
             dict(disp=ptr("disp") + 2), dict(free_row=ptr("free_row") + 1), dict(free_disp=ptr("free_disp") + 3), dict(n_rays=ptr("n_rays") + 2),
             dict(cells=ptr("cells") + 8), dict(cells=ptr("cells") + 4)]
    cases += [dict(XT=keep[k].ctypes.data) for k in range(4)] + [dict(spec=s_) for s_ in bad_specs]
    for kw in cases:
        rc, text = call(**kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_occupancy"), (sorted(kw), rc, text)
    assert call(batch=0) == 0 and call(batch=0, state=None, XR=None, XT=None) == 0
    assert all((b == 0x5A).all() for b in bufs.values())


def test_header_build_and_loader_agree(eng):
    """The header declares the spec's words in the order of the ctypes structure, the library exports the entries the header declares,
    and build.py lists the new sources and header."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct sv_occupancy_spec \{(.*?)\} sv_occupancy_spec;", src, flags=re.S).group(1)
    words = [w.strip() for decl in re.findall(r"(?:int32_t|double) ([^;]+);", body) for w in decl.split(",")]
    assert words == ["x_range[2]", "y_range[2]", "z_range[2]"] + [k for k, _ in eng.SvOccupancySpec._fields_[3:-1]] + ["reserved[5]"]
    declared = set(re.findall(r"\b(sv_[a-z_]*occupancy[a-z_]*)\s*\(", src))
    assert declared == {"sv_occupancy_dims", "sv_occupancy_disparity_device", "sv_debug_occupancy"}
    L = eng.occupancy_lib()
    assert all(hasattr(L, n) for n in declared) and len(L.sv_occupancy_disparity_device.argtypes) == 15
    build = util.pkg("build")
    assert "occupancy_kernels.hip" in build.SOURCES and "occupancy.cpp" in build.SOURCES and "occupancy_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("occupancy_kernels.hip", "occupancy.cpp", "occupancy_kernels.h"))
    assert "occupancy_grid" in util.pkg("stereo_vision.sv").__doc__


# ---------------------------------------------------------------------------------------------------------------- GPU

C2V = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
CLI_GRID = dict(x_range=(0, 40), y_range=(-20, 20), z_range=(-1.4, 1.0), scale=10)
# (XR, XT, grid): camera axes (X right, Y down, Z forward); the CLI's vehicle grid; a lifted and shifted frame - the scene lies around
# y = 30, so the grid does too - whose origin (-5, 30), cell (450, 200), lies 5 m behind the grid's near edge
FRAMES = {"camera": (None, None, dict(x_range=(-20, 20), y_range=(-3, 3), z_range=(0, 60), scale=6)),
          "vehicle": (C2V, None, CLI_GRID),
          "outside": (C2V, np.array([-5.0, 30.0, 1.65]), dict(x_range=(0, 40), y_range=(10, 50), z_range=(-0.5, 3.0), scale=10, z_scale=50, min_obstacle=5, min_rays=2))}


def _gpu(eng, d, lab, row, dsp, Q, XR=None, XT=None, **kw):
    """engine.occupancy_from_disparity on numpy batches -> dict of numpy arrays."""
    res = eng.occupancy_from_disparity(_cuda(np.asarray(d, np.float32)), _cuda(np.asarray(lab, np.uint8)), _cuda(np.asarray(row, np.int32)),
                                       _cuda(np.asarray(dsp, np.float32)), Q, XR=XR, XT=XT, **kw)
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in OUTPUTS}


def _want(sv, d, lab, row, dsp, Q, XR=None, XT=None, **kw):
    out = [sv.occupancy_grid(d[b], lab[b], row[b], dsp[b], Q, XR=XR, XT=XT, **kw) for b in range(len(d))]
    return {k: np.stack([o[k] for o in out]) for k in OUTPUTS}


def _check(sv, eng, d, lab, row, dsp, Q, XR=None, XT=None, **kw):
    got, want = _gpu(eng, d, lab, row, dsp, Q, XR, XT, **kw), _want(sv, d, lab, row, dsp, Q, XR, XT, **kw)
    for k in OUTPUTS:
        bad = [b for b in range(len(d)) if not _bits(got[k][b], want[k][b])]
        assert not bad, (k, bad, kw)
    return got


@pytest.fixture(scope="module")
def kitti(eng):
    """The seven committed KITTI frames 0 .. 6 through a rig: (d1, labels, free_row, free_disp) as numpy - the engine's d1, ground's
    outputs - and the rig's Q."""
    ls = [util.load_png("kitti0_color_left.png")] + [np.repeat(util.load_png("kitti%d_left.png" % k)[..., None], 3, -1) for k in range(1, 7)]
    rs = [util.load_png("kitti0_color_right.png")] + [np.repeat(util.load_png("kitti%d_right.png" % k)[..., None], 3, -1) for k in range(1, 7)]
    rig = util.pkg("rig").StereoRig(W, H)
    try:
        d1 = rig.disparity(_cuda(np.stack(ls)), _cuda(np.stack(rs)), pixel_format="rgb")
        g = eng.ground_from_disparity(d1, rig.params.disp_max, want_vdisp=False)
        Q = rig.Q.copy()
        out = tuple(t.cpu().numpy() for t in (d1, g.labels, g.free_row, g.free_disp))
        assert (g.ground.cpu().numpy()[:, 1] > 0).all()
    finally:
        rig.close()
    return out + (Q,)


@pytest.mark.gpu
def test_hand_built_map_on_the_gpu(sv, eng):
    for kw in (dict(min_obstacle=2), dict(), dict(z_scale=3), dict(XT=(0, 3, 0), min_obstacle=2)):
        _check(sv, eng, HAND_D[None], HAND_LABELS[None], HAND_FREE_ROW[None], HAND_FREE_DISP[None], HAND_Q, **dict(HAND_GRID, **kw))
    d, wall = _scene()
    g = sv.ground(d, 127)
    _check(sv, eng, d[None], g["labels"][None], g["free_row"][None], g["free_disp"][None], SCENE_Q, XR=C2V, **SCENE_GRID)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_kitti_frames_equal_the_definition(sv, eng, kitti, frame):
    d, lab, row, dsp, Q = kitti
    XR, XT, grid = FRAMES[frame]
    batch = _check(sv, eng, d, lab, row, dsp, Q, XR, XT, **grid)
    occupied, free, rays = [(batch["state"] == k).sum(axis=(1, 2)) for k in (2, 1)] + [batch["n_rays"].sum(axis=(1, 2))]
    print("%s: occupied %s, free %s, ray cells %s" % (frame, occupied.tolist(), free.tolist(), rays.tolist()))
    assert (occupied > 0).all() and (free > 0).all() and (rays > 0).all()
    for b in range(len(d)):  # each alone
        alone = _gpu(eng, d[b:b + 1], lab[b:b + 1], row[b:b + 1], dsp[b:b + 1], Q, XR, XT, **grid)
        assert all(_bits(alone[k][0], batch[k][b]) for k in OUTPUTS), (frame, b)
    for shift in range(1, len(d)):  # and at each position of a batch
        roll = lambda a: np.roll(a, shift, axis=0)  # noqa: E731
        moved = _gpu(eng, roll(d), roll(lab), roll(row), roll(dsp), Q, XR, XT, **grid)
        assert all(_bits(moved[k], roll(batch[k])) for k in OUTPUTS), (frame, shift)


def _raw(eng, t, spec, rows, cols, Q, XR, XT, fill=0xA5, state=True):
    """The C entry on caller-owned, pre-filled outputs."""
    import torch
    d, lab, row, dsp = t
    B, Hh, Ww = d.shape
    cells = torch.full((B, rows, cols, 4), fill, dtype=torch.uint8, device="cuda").repeat_interleave(4, -1).view(torch.int32)
    n_rays = torch.full((B, rows, cols, 4), fill, dtype=torch.uint8, device="cuda").view(torch.int32).squeeze(-1)
    st = torch.full((B, rows, cols), fill, dtype=torch.uint8, device="cuda")
    assert tuple(cells.shape) == (B, rows, cols, 4) and tuple(n_rays.shape) == (B, rows, cols)
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    xr = None if XR is None else np.ascontiguousarray(XR, np.float64).reshape(9)
    xt = None if XT is None else np.ascontiguousarray(XT, np.float64).reshape(3)
    rc = eng.occupancy_lib().sv_occupancy_disparity_device(d.data_ptr(), lab.data_ptr(), row.data_ptr(), dsp.data_ptr(), B, Ww, Hh, q.ctypes.data,
                                                           None if xr is None else xr.ctypes.data, None if xt is None else xt.ctypes.data, ctypes.byref(spec),
                                                           cells.data_ptr(), n_rays.data_ptr(), st.data_ptr() if state else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, eng.occupancy_lib().sv_last_error(None))
    torch.cuda.synchronize()
    return {"cells": cells.cpu().numpy(), "n_rays": n_rays.cpu().numpy(), "state": st.cpu().numpy()}


@pytest.mark.gpu
def test_prefilled_outputs_repeats_and_combine(sv, eng, kitti):
    """Outputs full of 0xA5, five repeats, the wave combine on and off: the same bits every time, and fewer atomics with the combine."""
    import torch
    d, lab, row, dsp, Q = kitti
    t = tuple(_cuda(a) for a in (d, lab, row, dsp))
    XR, XT, grid = FRAMES["vehicle"]
    spec, rows, cols = eng.occupancy_spec(**grid)
    want = _gpu(eng, d, lab, row, dsp, Q, XR, XT, **grid)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    issued = {}
    try:
        for combine in (1, 0):
            for rep in range(5):
                counter.zero_()
                torch.cuda.synchronize()
                assert eng.debug_occupancy(combine, counter) == 0
                got = _raw(eng, t, spec, rows, cols, Q, XR, XT)
                assert all(_bits(got[k], want[k]) for k in OUTPUTS), (combine, rep)
                issued.setdefault(combine, set()).add(int(counter.item()))
    finally:
        eng.debug_occupancy(True, None)
    kept = int(want["cells"][..., :2].sum())
    print("kept pixels %d, atomics issued without / with the combine: %s / %s" % (kept, sorted(issued[0]), sorted(issued[1])))
    assert issued[0] == {3 * kept} and len(issued[1]) == 1 and 0 < min(issued[1]) < 3 * kept
    # state NULL: the byte buffer stays as it was, the rest is the same
    got = _raw(eng, t, spec, rows, cols, Q, XR, XT, state=False)
    assert (got["state"] == 0xA5).all() and _bits(got["cells"], want["cells"]) and _bits(got["n_rays"], want["n_rays"])
    no_state = eng.occupancy_from_disparity(*t, Q, XR=XR, want_state=False, **grid)
    assert no_state.state is None and _bits(no_state.cells.cpu().numpy(), want["cells"])


@pytest.mark.gpu
def test_degenerate_frames(sv, eng, kitti):
    import torch
    d, lab, row, dsp, Q = kitti
    XR, XT, grid = FRAMES["vehicle"]
    h, w = 90, 200
    rng = np.random.default_rng(73)
    # all invalid (with labels that would count), no ground (every valid pixel 3, no free-space row), and a live frame between them
    dd = np.stack([rng.choice(np.array([NAN, -10.0, 0.0, -INF], np.float32), (h, w)), d[0, :h, :w], d[1, :h, :w], d[0, 100:100 + h, :w]])
    ll = np.stack([rng.integers(1, 3, (h, w)).astype(np.uint8), np.where(d[0, :h, :w] > 0, 3, 0).astype(np.uint8), lab[1, :h, :w], lab[0, 100:100 + h, :w]])
    rr = np.stack([np.full(w, -1, np.int32), np.full(w, -1, np.int32), np.full(w, -1, np.int32), np.clip(row[0, :w] - 100, -1, h - 1).astype(np.int32)])
    fd = np.stack([np.zeros(w, np.float32), np.zeros(w, np.float32), np.zeros(w, np.float32), dsp[0, :w]])
    got = _check(sv, eng, dd, ll, rr, fd, Q, XR, XT, **grid)
    for b in (0, 1):
        assert not got["state"][b].any() and not got["n_rays"][b].any() and (got["cells"][b] == [0, 0, -1, -1]).all()
    assert got["state"][3].any() and got["n_rays"][3].any()
    # free-space rows outside the map and disparities that are no disparities: arithmetic only, nothing is read through them
    rr2 = np.stack([np.full(w, 10 ** 9, np.int32), np.full(w, 2 ** 31 - 1, np.int32), rng.integers(0, 4 * h, w).astype(np.int32), rr[3]])
    fd2 = np.stack([fd[3], rng.choice(np.array([NAN, 0.0, -3.0, INF, 1e-30, 1e30], np.float32), w), np.abs(fd[3]) + 1, fd[3]])
    _check(sv, eng, dd, ll, rr2, fd2, Q, XR, XT, **grid)
    # every pixel in one cell: a Q that sends every pixel to (12.34, -3.21, 0.25), whatever its disparity
    one = np.array([[0, 0, 0, 12.34], [0, 0, 0, -3.21], [0, 0, 0, 0.25], [0, 0, 0, 1.0]])
    l1 = rng.integers(0, 4, (2, h, w)).astype(np.uint8)
    d1 = np.where(rng.random((2, h, w)) < 0.9, rng.uniform(0.5, 60, (2, h, w)), -10).astype(np.float32)
    r1 = np.stack([np.where(np.arange(w) % 3 == 0, -1, 5).astype(np.int32), np.full(w, -1, np.int32)])
    got = _check(sv, eng, d1, l1, r1, np.ones((2, w), np.float32), one, None, None, **grid)
    cell = got["cells"][:, 400 - 123, 200 + 32]
    assert (got["cells"][..., :2].sum(axis=(1, 2)) == cell[:, :2]).all() and cell[:, 0].min() > 3000 and (cell[:, 2] == cell[:, 3]).all() and cell[0, 2] in (32, 33)
    # B = 0, and one frame without a batch axis
    t = [_cuda(a) for a in (dd, ll, rr, fd)]
    res = eng.occupancy_from_disparity(t[0][:0], t[1][:0], t[2][:0], t[3][:0], Q, XR=XR, **grid)
    assert tuple(res.cells.shape) == (0, 401, 401, 4) and tuple(res.n_rays.shape) == (0, 401, 401) and tuple(res.state.shape) == (0, 401, 401)
    single = eng.occupancy_from_disparity(t[0][3], t[1][3], t[2][3], t[3][3], Q, XR=XR, **grid)
    live = _gpu(eng, dd, ll, rr, fd, Q, XR, **grid)["state"][3]
    assert tuple(single.state.shape) == (1, 401, 401) and live.any() and torch.equal(single.state[0], _cuda(live))
    for bad in (dict(d1=t[0].double()), dict(d1=t[0].cpu()), dict(labels=t[1].int()), dict(free_row=t[2][:, :-1]), dict(free_disp=t[3].cpu()), dict(scale=0),
                dict(z_scale=0), dict(min_rays=0), dict(XT=(1e9, 0, 0))):
        a = dict(dict(d1=t[0], labels=t[1], free_row=t[2], free_disp=t[3], Q=Q, XR=XR), **grid)
        with pytest.raises(ValueError):
            eng.occupancy_from_disparity(**dict(a, **bad))


@pytest.mark.gpu
def test_arithmetic_edges(sv, eng):
    """Points a few ulps around the cell edges, the height steps and the range bounds.  With Q below and w = 1 a pixel (x, y) of disparity
    d lies at X = fl(fl(x / 7) + ex), Y = fl(fl(y / 7) + (ey - 3)), Z = fl(fl(d / 7) + (ez - 1)): x = 0 .. 42 walks over every cell edge k / 7
    of x 0..6 at scale 7 and ends on both bounds, y does the same for y -3..3, and d = 1 .. 14 for the height steps of z -1..1 at z_scale 7;
    ex, ey, ez shift everything by a few ulps.  One pixel per cell, so nothing hides behind a sum."""
    n = 43
    x, y = np.meshgrid(np.arange(n), np.arange(n))
    d = ((x + 3 * y) % 14 + 1).astype(np.float32)
    lab = ((x + y) % 2 + 1).astype(np.uint8)
    row = np.where(np.arange(n) % 2 == 0, (np.arange(n) * 5) % n, -1).astype(np.int32)
    dsp = ((np.arange(n) % 14) + 1).astype(np.float32)
    grid = dict(x_range=(0, 6), y_range=(-3, 3), z_range=(-1, 1), scale=7, z_scale=7)
    seen = set()
    for m in (-4, -2, -1, 0, 1, 2, 4):
        for ex, ey, ez in ((m, m, m), (m, -m, 0), (0, m, -m)):
            Q = np.array([[1 / 7, 0, 0, ex * 2.0 ** -52], [0, 1 / 7, 0, -3 + ey * 2.0 ** -52], [0, 0, 1 / 7, -1 + ez * 2.0 ** -53], [0, 0, 0, 1.0]])
            got = _check(sv, eng, d[None], lab[None], row[None], dsp[None], Q, **grid)
            assert got["cells"][0, ..., :2].sum() > 0.7 * n * n
            seen.add(got["cells"].tobytes())
    assert len(seen) > 2  # the shifts do move points over edges: downward, none and upward give different grids at the least


@pytest.mark.gpu
def test_rig_occupancy(sv, eng):
    import torch
    rigmod = util.pkg("rig")
    ls = np.stack([util.load_png("kitti0_color_left.png"), np.repeat(util.load_png("kitti1_left.png")[..., None], 3, -1)])
    rs = np.stack([util.load_png("kitti0_color_right.png"), np.repeat(util.load_png("kitti1_right.png")[..., None], 3, -1)])
    bgr_l, bgr_r = np.ascontiguousarray(ls[..., ::-1]), np.ascontiguousarray(rs[..., ::-1])
    rig = rigmod.StereoRig(W, H)
    try:
        tl, tr = _cuda(bgr_l), _cuda(bgr_r)
        res = rig.occupancy(tl, tr, transform=(sv.CAMERA_TO_VEHICLE, None), **CLI_GRID)
        d1 = rig.disparity(tl, tr)
        g = eng.ground_from_disparity(d1, rig.params.disp_max, want_vdisp=False)
        ref = eng.occupancy_from_disparity(d1, g.labels, g.free_row, g.free_disp, rig.Q, XR=sv.CAMERA_TO_VEHICLE, **CLI_GRID)
        for k in OUTPUTS:
            assert isinstance(getattr(res, k), torch.Tensor) and torch.equal(getattr(res, k), getattr(ref, k)), k
        for k in ("ground", "labels", "free_row", "free_disp"):
            assert torch.equal(getattr(res.ground, k), getattr(g, k)), k
        assert res.ground.vdisp is None and res.spec.z_scale == 20 and (res.state == 2).sum().item() > 100
        # the definition on the same maps
        want = sv.occupancy_grid(d1[0].cpu().numpy(), g.labels[0].cpu().numpy(), g.free_row[0].cpu().numpy(), g.free_disp[0].cpu().numpy(), rig.Q,
                                 XR=sv.CAMERA_TO_VEHICLE, **CLI_GRID)
        assert all(_bits(getattr(res, k)[0].cpu().numpy(), want[k]) for k in OUTPUTS)
        # numpy in: numpy out; spec words of both stages pass through
        XT = np.array([0.0, 0.0, 1.65])
        out = rig.occupancy(bgr_l, bgr_r, (0, 40), (-20, 20), (0.2, 3.0), 5, transform=(sv.CAMERA_TO_VEHICLE, XT), ground=dict(vh_step=4, qb_step=4, min_run=4),
                            z_scale=10, min_obstacle=6, want_state=False)
        g2 = eng.ground_from_disparity(d1, rig.params.disp_max, vh_step=4, qb_step=4, min_run=4)
        ref = eng.occupancy_from_disparity(d1, g2.labels, g2.free_row, g2.free_disp, rig.Q, (0, 40), (-20, 20), (0.2, 3.0), 5, XR=sv.CAMERA_TO_VEHICLE, XT=XT, z_scale=10,
                                           min_obstacle=6)
        assert out.state is None and isinstance(out.cells, np.ndarray) and isinstance(out.ground.labels, np.ndarray)
        assert _bits(out.cells, ref.cells.cpu().numpy()) and _bits(out.n_rays, ref.n_rays.cpu().numpy()) and _bits(out.ground.free_row, g2.free_row.cpu().numpy())
        for bad in (dict(scale=0), dict(z_scale=0), dict(min_rays=0), dict(transform="sideways"), dict(ground=dict(tol=17)), dict(ground=dict(want_free=False)),
                    dict(ground=dict(n_bins=64)), dict(transform=(None, (1e9, 0, 0)))):
            with pytest.raises(ValueError):
                rig.occupancy(bgr_l, bgr_r, **dict(dict(CLI_GRID), **bad))
    finally:
        rig.close()
    p = util.pkg("engine").SvParams.driver(255)
    p.subsampling = 1
    half = rigmod.StereoRig(W, H, params=p)
    try:
        with pytest.raises(ValueError):
            half.occupancy(bgr_l, bgr_r, **CLI_GRID)
    finally:
        half.close()


@pytest.mark.gpu
def test_cli_occupancy_writes_one_png_per_pair(sv, tmp_path):
    from PIL import Image
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    frames = [(util.load_png("kitti0_color_left.png"), util.load_png("kitti0_color_right.png"))]
    for k in (1, 2):
        frames.append(tuple(np.repeat(util.load_png("kitti%d_%s.png" % (k, s))[..., None], 3, -1) for s in ("left", "right")))
    for i, (l, r) in enumerate(frames):
        Image.fromarray(l).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(r).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with pytest.raises(SystemExit):
        sv.main(["-k", str(tmp_path / "kitti"), "--occupancy", str(tmp_path / "occ")])  # needs --batch
    sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--occupancy", str(tmp_path / "occ")])
    rig = util.pkg("rig").StereoRig(W, H)
    try:
        want = rig.occupancy(np.stack([l for l, _ in frames]), np.stack([r for _, r in frames]), pixel_format="rgb", transform=(sv.CAMERA_TO_VEHICLE, None),
                             **sv.CLI_TOP_VIEW).state
    finally:
        rig.close()
    assert sorted(os.listdir(tmp_path / "occ")) == ["%010d.png" % i for i in range(len(frames))]
    for i in range(len(frames)):
        got = np.asarray(Image.open(tmp_path / "occ" / ("%010d.png" % i)))
        assert got.shape == (401, 401) and set(np.unique(got).tolist()) == {0, 127, 255} and np.array_equal(got, np.array([0, 127, 255], np.uint8)[want[i]]), i
