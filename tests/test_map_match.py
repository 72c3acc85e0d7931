"""The correlative match of occupancy frames against the world map (include/stereo_vision_hip.h (L)): the numpy definition in stereo_vision.sv
on hand-computed cases, its agreement with the fuse, the recovery of a known pose, ties, the argument checks in Python and in the C ABI, and
the HIP kernels - C entry, engine, rig.OccupancyMap.match / localize and the CLI's --match - against the definition.

Everything is compared exactly.  That is derived, not chosen: a frame cell's point, its place in the world and the range tests are products,
sums and comparisons of doubles in a stated order - -ffp-contract=off on the device, and numpy never fuses - and everything behind floor() is
a sum of integers, which does not depend on the order of the additions."""
import ctypes
import os
import re

import numpy as np
import pytest

import map_stage_cases as mc
import util
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_occupancy_map import CLI_GRID, DRIVE_MAP, _drive_frames, drive  # noqa: F401 (drive: the committed KITTI frames' states, a fixture)

SV_ERR_ARG = -1
NAN, INF = float("nan"), float("inf")
KEYS = ("sums", "counts", "score", "best", "best_score")
DTYPES = dict(sums=np.int64, counts=np.int32, score=np.int64, best=np.int32, best_score=np.int64)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _same(got, want):
    return all(_bits(got[k], want[k]) for k in KEYS)


# ---------------------------------------------------------------------------------------------------------------- CPU

# A frame grid of 3 x 3 cells: x 0..2, y -1..1 at scale 1, so FR1 = 2, FC1 = 1 and hf = 0.5.  Rows 0, 1, 2 have kx = 2, 1, 0 and stand for
# Xf = 2.5, 1.5, 0 (the double-width cell at 0 is 0); columns 0, 1, 2 have ky = 1, 0, -1 and stand for Yf = 1.5, 0, -1.5.
HAND_FRAME = dict(x_range=(0, 2), y_range=(-1, 1), scale=1)
HAND_STATE = np.array([[2, 1, 0],
                       [0, 2, 1],
                       [1, 3, 2]], np.uint8)
# The map x 0..4, y -2..2 at scale 1: top 4, left 2, 4 x 4 cells; the world point (Xw, Yw) lies in cell (3 - floor(Xw), 1 - floor(Yw)).
HAND_MAP = dict(top=4, left=2, rows=4, cols=4, scale=1, l_occ=85, l_free=40, l_min=-200, l_max=350)
HAND_LOGODDS = np.array([[1, 2, 3, 4],
                         [5, -6, 7, 8],
                         [9, 10, -11, 12],
                         [13, 14, 15, 16]], np.int16)
# identity   occupied (2.5, 1.5) -> (1, 0) = 5, (1.5, 0) -> (2, 1) = 10, (0, -1.5) -> (3, 3) = 16: H = 31 of 3;
#            free (2.5, 0) -> (1, 1) = -6, (1.5, -1.5) -> (2, 3) = 12, (0, 1.5) -> (3, 0) = 13: M = 19 of 3.
# t = (1, 0) occupied (3.5, 1.5) -> (0, 0) = 1, (2.5, 0) -> (1, 1) = -6, (1, -1.5) -> (2, 3) = 12: H = 7; free (3.5, 0) -> (0, 1) = 2,
#            (2.5, -1.5) -> (1, 3) = 8, (1, 1.5) -> (2, 0) = 9: M = 19.
# t = (2, 0) occupied (4.5, .) has gx = 4 > top - 1: out, (3.5, 0) -> (0, 1) = 2, (2, -1.5) -> (1, 3) = 8: H = 10 of 2; free (4.5, .) out,
#            (3.5, -1.5) -> (0, 3) = 4, (2, 1.5) -> (1, 0) = 5: M = 9 of 2.
# quarter    (c, s) = (0, 1): Xw = -Yf, Yw = Xf.  Occupied (-1.5, 2.5) out, (0, 1.5) -> (3, 0) = 13, (1.5, 0) -> (2, 1) = 10: H = 23 of 2; free
#            (0, 2.5) has gy = 2 > left - 1: out, (1.5, 1.5) -> (2, 0) = 9, (-1.5, 0) out: M = 9 of 1.
HAND_POSES = [(0.0, 0.0, 1.0, 0.0), (1.0, 0.0, 1.0, 0.0), (2.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0)]
HAND_SUMS = [(31, 19), (7, 19), (10, 9), (23, 9)]
HAND_COUNTS = [(3, 3), (3, 3), (2, 2), (2, 1)]


def test_hand_computed_case(sv):
    got = sv.occupancy_match(HAND_STATE, HAND_POSES, HAND_FRAME, HAND_MAP, HAND_LOGODDS, w_occ=2, w_free=1)
    assert all(got[k].dtype == DTYPES[k] for k in KEYS)
    assert got["sums"].shape == (1, 4, 2) and got["sums"][0].tolist() == [list(v) for v in HAND_SUMS]
    assert got["counts"][0].tolist() == [list(v) for v in HAND_COUNTS]
    assert got["score"][0].tolist() == [43, -5, 11, 37] and got["best"].tolist() == [0] and got["best_score"].tolist() == [43]
    # without the free cells: they are not visited
    occ = sv.occupancy_match(HAND_STATE[None], np.array([HAND_POSES]), HAND_FRAME, HAND_MAP, HAND_LOGODDS)
    assert occ["sums"][0].tolist() == [[h, 0] for h, _ in HAND_SUMS] and occ["counts"][0].tolist() == [[n, 0] for n, _ in HAND_COUNTS]
    assert occ["score"][0].tolist() == [31, 7, 10, 23] and occ["best_score"].tolist() == [31]
    # the free cells alone, and the largest weights
    free = sv.occupancy_match(HAND_STATE, HAND_POSES, HAND_FRAME, HAND_MAP, HAND_LOGODDS, w_occ=0, w_free=32767)
    assert free["score"][0].tolist() == [-19 * 32767, -19 * 32767, -9 * 32767, -9 * 32767] and free["best"].tolist() == [2]
    # logodds as stored: the whole int16 range, outside l_min .. l_max
    wide = np.where(HAND_LOGODDS > 0, 32767, -32768).astype(np.int16)
    assert sv.occupancy_match(HAND_STATE, HAND_POSES, HAND_FRAME, HAND_MAP, wide, 1, 1)["sums"][0, 0].tolist() == [3 * 32767, 2 * 32767 - 32768]


def test_cell_points_and_the_trunc_identity(sv):
    Xf, Yf = sv.occupancy_frame_points(HAND_FRAME)
    assert Xf.tolist() == [2.5, 1.5, 0.0] and Yf.tolist() == [1.5, 0.0, -1.5]  # k = 0 stands for 0
    for grid in (HAND_FRAME, dict(x_range=(0, 12), y_range=(-6, 6), scale=4), dict(x_range=(-3, 5), y_range=(-7, -2), scale=3), CLI_GRID,
                 dict(x_range=(2, 9), y_range=(1, 4), scale=7), dict(x_range=(-1000003, -1000000), y_range=(2 ** 31 - 4, 2 ** 31), scale=10)):
        (fx0, fx1), (fy0, fy1), scale, rows, cols = sv.occupancy_frame_grid(grid)
        Xf, Yf = sv.occupancy_frame_points(grid)
        assert Xf.shape == (rows,) and Yf.shape == (cols,)
        fs = float(scale)
        kx = int(np.trunc(fx1 * fs)) - np.arange(rows)
        ky = int(np.trunc(fy1 * fs)) - np.arange(cols)
        # the fuse would look the point up in the cell it stands for
        assert np.array_equal(np.trunc(Xf * fs), kx) and np.array_equal(np.trunc(Yf * fs), ky), grid
        assert (Xf[kx == 0] == 0).all() and (Yf[ky == 0] == 0).all()
        assert np.array_equal(Xf, (2 * kx + np.sign(kx)).astype(np.float64) * (1.0 / (2.0 * fs)))  # one product by hf, no division per cell


def test_agrees_with_the_fuse(sv):
    """One frame fused into a fresh map at zero yaw and a whole-cell translation, then matched there: every occupied cell the fuse can see
    lands on a cell that took exactly l_occ.  (The fuse sees a cell iff its centre lies strictly inside the frame's ranges: the frame's
    first row and its first and last column - kx = FR1, ky = FC1 and ky = trunc(fy0 fs) - lie outside, so the state leaves them empty.)"""
    frame = dict(x_range=(0, 8), y_range=(-2, 2), scale=2)
    words = sv.occupancy_map_params((-5, 20), (-10, 10), 2, l_occ=77, l_free=31)
    rng = np.random.default_rng(3)
    state = rng.integers(0, 3, (17, 9)).astype(np.uint8)
    state[0] = state[:, 0] = state[:, -1] = 0
    for t in ((0.0, 0.0), (3.5, -2.0), (-4.0, 5.5)):
        pose = sv.occupancy_pose(t[0], t[1], 0.0)
        fused = sv.occupancy_fuse(state, [pose], frame, words)
        got = sv.occupancy_match(state, [pose], frame, words, fused["logodds"], 1, 1)
        n_occ, n_free = int((state == 2).sum()), int((state == 1).sum())
        assert n_occ > 10 and got["counts"][0, 0].tolist() == [n_occ, n_free]
        assert got["sums"][0, 0].tolist() == [n_occ * 77, -n_free * 31], t


RECOVERY_FRAME = dict(x_range=(0, 12), y_range=(-6, 6), scale=4)
RECOVERY_MAP = dict(x_range=(-10, 30), y_range=(-20, 20), scale=4)
RECOVERY_WINDOW = ((0.75, 0.75, 0.04), (7, 7, 5))  # steps of 0.25 m and 0.02 rad


def _recovery_state():
    """49 x 49: an L-shaped wall, a post and a block in free space, the far rows unknown."""
    st = np.ones((49, 49), np.uint8)
    st[5:40, 10] = 2
    st[5, 10:35] = 2
    st[25, 30] = 2
    st[30:34, 38:42] = 2
    st[:3] = 0
    return st


@pytest.mark.parametrize("yaw", [0.0, 0.3, -1.1])
@pytest.mark.parametrize("w_free", [0, 1])
def test_recovers_the_pose_it_was_fused_at(sv, yaw, w_free):
    state = _recovery_state()
    assert state.shape == sv.occupancy_frame_grid(RECOVERY_FRAME)[3:]
    words = sv.occupancy_map_params(**RECOVERY_MAP)
    assert (words["rows"], words["cols"]) == (160, 160)
    fused = sv.occupancy_fuse(state, [sv.occupancy_pose(3.25, -1.5, yaw)], RECOVERY_FRAME, words)
    # around p* itself: index 0; and around a guess one step off in x and two in y, where p* is window cell (4, 1, 2) - behind the middle one, so its row is its row-major index
    for guess, at in (((3.25, -1.5, yaw), 0), ((3.0, -1.0, yaw), (4 * 7 + 1) * 5 + 2)):
        window = sv.occupancy_pose_window(*guess, *RECOVERY_WINDOW)
        assert window.shape == (245, 3) and window[at].tolist() == [3.25, -1.5, yaw]
        got = sv.occupancy_match(state, sv.occupancy_pose(window[:, 0], window[:, 1], window[:, 2]), RECOVERY_FRAME, words, fused["logodds"], 1, w_free)
        top = np.sort(got["score"][0])[::-1]
        print("yaw %r w_free %d: best %d with %d, runner-up %d" % (yaw, w_free, got["best"][0], top[0], top[1]))
        assert got["best"].tolist() == [at] and got["best_score"].tolist() == [top[0]] and top[0] > top[1]


def test_ties_empty_frames_and_poses_that_miss(sv):
    words = sv.occupancy_map_params(**RECOVERY_MAP)
    rng = np.random.default_rng(5)
    logodds = rng.integers(-200, 351, (160, 160)).astype(np.int16)
    state = _recovery_state()
    good = sv.occupancy_pose(3.25, -1.5, 0.3)
    other = sv.occupancy_pose(2.0, 1.0, -0.2)
    one = sv.occupancy_match(state, [good, other], RECOVERY_FRAME, words, logodds, 1, 1)
    assert one["score"][0, 0] != one["score"][0, 1] and one["counts"].min() > 0
    hi, lo = (good, other) if one["score"][0, 0] > one["score"][0, 1] else (other, good)
    # the same pose several times: the lowest index of the largest score
    tied = sv.occupancy_match(state, [lo, hi, lo, hi, hi], RECOVERY_FRAME, words, logodds, 1, 1)
    assert tied["best"].tolist() == [1] and tied["score"][0, 1] == tied["score"][0, 3] == tied["score"][0, 4]
    # a frame without a cell, and one with bytes that play no part: all 0, best 0
    for empty in (np.zeros((49, 49), np.uint8), np.full((49, 49), 3, np.uint8), np.full((49, 49), 255, np.uint8)):
        got = sv.occupancy_match(empty, [lo, hi, hi], RECOVERY_FRAME, words, logodds, 1, 1)
        assert not got["sums"].any() and not got["counts"].any() and got["best"].tolist() == [0] and got["best_score"].tolist() == [0]
    # free cells alone with w_free == 0: the same
    got = sv.occupancy_match(np.ones((49, 49), np.uint8), [lo, hi], RECOVERY_FRAME, words, logodds, 1, 0)
    assert not got["sums"].any() and not got["counts"].any() and got["best"].tolist() == [0]
    # a word that is not finite, or a frame wholly outside the map: 0 of 0
    poses = [good]
    for k in range(4):
        for bad in (NAN, INF, -INF):
            pose = list(good)
            pose[k] = bad
            poses.append(pose)
    poses += [(1000.0, 0.0, 1.0, 0.0), (0.0, -1e300, 0.0, 1.0), (31.0, 0.0, 1.0, 0.0), (-22.5, 0.0, 1.0, 0.0), (0.0, 26.5, 1.0, 0.0), (0.0, -26.5, 1.0, 0.0)]
    got = sv.occupancy_match(state, poses, RECOVERY_FRAME, words, logodds, 3, 2)
    assert not got["sums"][0, 1:].any() and not got["counts"][0, 1:].any() and got["counts"][0, 0].tolist() == [int((state == 2).sum()), int((state == 1).sum())]
    # one cell less far away and the frame's edge is back in the map
    edge = sv.occupancy_match(state, [(29.75, 0.0, 1.0, 0.0), (0.0, 25.75, 1.0, 0.0)], RECOVERY_FRAME, words, logodds, 1, 1)
    assert (edge["counts"].sum(-1) > 0).all()


def test_pose_window(sv):
    w = sv.occupancy_pose_window(1.0, -2.0, 0.5, (0.5, 0.25, 0.1), (3, 5, 3))
    assert w.dtype == np.float64 and w.shape == (45, 3) and w[0].tolist() == [1.0, -2.0, 0.5]
    xs, ys, yaws = 1.0 + np.linspace(-0.5, 0.5, 3), -2.0 + np.linspace(-0.25, 0.25, 5), 0.5 + np.linspace(-0.1, 0.1, 3)
    plain = [[xs[i], ys[j], yaws[k]] for i in range(3) for j in range(5) for k in range(3) if (i, j, k) != (1, 2, 1)]
    assert w[1:].tolist() == plain and len(plain) == 44
    assert sv.occupancy_pose_window(1.0, 2.0, 3.0, (9, 9, 9), (1, 1, 1)).tolist() == [[1.0, 2.0, 3.0]]
    only_yaw = sv.occupancy_pose_window(0.0, 0.0, 0.0, (1, 1, 0.25), (1, 1, 5))
    assert only_yaw[:, 2].tolist() == [0.0, -0.25, -0.125, 0.125, 0.25] and not only_yaw[:, :2].any()
    assert sv.occupancy_pose_window(0, 0, 0, (0, 0, 0), (255, 257, 1)).shape == (65535, 3)
    for bad in (dict(steps=(2, 1, 1)), dict(steps=(3, 0, 1)), dict(steps=(3, 3)), dict(steps=(3, 1.5, 1)), dict(steps=(True, 1, 1)), dict(steps=(257, 257, 1)),
                dict(half=(1, 1)), dict(half=(-1, 0, 0)), dict(half=(NAN, 0, 0)), dict(half=(0, INF, 0)), dict(x=NAN), dict(yaw=INF)):
        with pytest.raises(ValueError):
            sv.occupancy_pose_window(**dict(dict(x=0.0, y=0.0, yaw=0.0, half=(1, 1, 0.1), steps=(3, 3, 3)), **bad))


_BAD_MAPS = [dict(rows=0), dict(cols=40000), dict(scale=0), dict(top=2 ** 24), dict(left=-2 ** 24), dict(l_occ=0), dict(l_free=40000), dict(l_min=1), dict(l_max=32768),
             dict(l_min=0, l_max=0)]
_BAD_FRAMES = [dict(x_range=(0.5, 2)), dict(x_range=(2, 2)), dict(y_range=(1, -1)), dict(scale=0), dict(x_range=(0, 40000))]
_BAD_WEIGHTS = [dict(w_occ=-1), dict(w_occ=32768), dict(w_free=-1), dict(w_free=32768), dict(w_occ=0, w_free=0)]


def _c_map(eng, reserved=None, **kw):
    sp = eng.SvOccupancyMapSpec()
    for k, v in dict(HAND_MAP, **kw).items():
        setattr(sp, k, v)
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


def test_validation_needs_no_device(sv, eng):
    """Every refused argument raises ValueError in Python; the C entry returns SV_ERR_ARG on host buffers, which stay untouched: the checks
    run before any HIP call."""
    base = dict(state=HAND_STATE, poses=HAND_POSES, frame_grid=HAND_FRAME, map=HAND_MAP, logodds=HAND_LOGODDS)
    bad_args = [dict(map=dict(HAND_MAP, **kw)) for kw in _BAD_MAPS] + [dict(frame_grid=dict(HAND_FRAME, **kw)) for kw in _BAD_FRAMES] + _BAD_WEIGHTS
    bad_args += [dict(w_occ=1.5), dict(w_free=True), dict(state=HAND_STATE[:2]), dict(state=HAND_STATE.astype(np.int32)), dict(poses=[p[:3] for p in HAND_POSES]),
                 dict(poses=np.zeros((2, 4, 4))), dict(poses=np.zeros((1, 0, 4))), dict(poses=np.zeros((1, 65536, 4))), dict(logodds=HAND_LOGODDS.astype(np.int32)),
                 dict(logodds=HAND_LOGODDS[:3])]
    for bad in bad_args:
        with pytest.raises(ValueError):
            sv.occupancy_match(**dict(base, **bad))

    L = eng.map_match_lib()
    frame, _, _ = eng.occupancy_spec((0, 2), (-1, 1), (-1, 1), 1)
    need = ctypes.c_size_t(0)
    assert L.sv_map_match_workspace(ctypes.byref(frame), 2, 0, ctypes.byref(need)) == 0 and need.value >= 2 * 9 * 4 and need.value % 16 == 0
    per_frame = need.value // 2
    sizes = []
    for batch in (0, 1, 2, 7, 65535):
        for w_free in (0, 1):
            assert L.sv_map_match_workspace(ctypes.byref(frame), batch, w_free, ctypes.byref(need)) == 0 and need.value >= batch * 9 * 4 and need.value % 16 == 0
            sizes.append(need.value)
    assert sizes[0] == 0 and sizes == sorted(sizes)
    bufs = {k: np.full(2 * per_frame + 64, 0x5A, np.uint8) for k in ("state", "poses", "logodds", "sums", "counts", "best", "best_score", "ws")}
    ptr = lambda name: bufs[name].ctypes.data + (-bufs[name].ctypes.data) % 16  # noqa: E731
    base = dict(state=ptr("state"), poses=ptr("poses"), batch=2, n_poses=4, frame=frame, map=_c_map(eng), logodds=ptr("logodds"), w_occ=1, w_free=1, sums=ptr("sums"),
                counts=ptr("counts"), best=ptr("best"), best_score=ptr("best_score"), ws=ptr("ws"), ws_bytes=2 * per_frame)

    def call(**kw):
        a = dict(base, **kw)
        return L.sv_map_match_device(a["state"], a["poses"], a["batch"], a["n_poses"], None if a["frame"] is None else ctypes.byref(a["frame"]),
                                     None if a["map"] is None else ctypes.byref(a["map"]), a["logodds"], a["w_occ"], a["w_free"], a["sums"], a["counts"], a["best"],
                                     a["best_score"], a["ws"], a["ws_bytes"], None)

    bad_frames = []
    for kw in _BAD_FRAMES:
        f, _, _ = eng.occupancy_spec((0, 2), (-1, 1), (-1, 1), 1)
        for k, v in kw.items():
            if k == "scale":
                f.scale = v
            else:
                getattr(f, k)[:] = [float(t) for t in v]
        bad_frames.append(f)
    f, _, _ = eng.occupancy_spec((0, 2), (-1, 1), (-1, 1), 1)
    f.reserved[2] = 1
    bad_frames.append(f)
    cases = [dict(frame=None), dict(map=None), dict(state=None), dict(poses=None), dict(logodds=None), dict(ws=None), dict(sums=None), dict(counts=None), dict(best=None),
             dict(best_score=None), dict(sums=None, counts=None, best=None, best_score=None),
             dict(poses=ptr("poses") + 4), dict(logodds=ptr("logodds") + 1), dict(sums=ptr("sums") + 4), dict(counts=ptr("counts") + 2), dict(best=ptr("best") + 1),
             dict(best_score=ptr("best_score") + 4), dict(ws=ptr("ws") + 8), dict(ws_bytes=2 * per_frame - 1), dict(ws_bytes=0),
             dict(batch=-1), dict(batch=65536), dict(n_poses=0), dict(n_poses=-3), dict(n_poses=65536), dict(batch=65535, n_poses=32769, ws_bytes=2 ** 62)]
    cases += _BAD_WEIGHTS + [dict(frame=f) for f in bad_frames] + [dict(map=_c_map(eng, **kw)) for kw in _BAD_MAPS] + [dict(map=_c_map(eng, reserved=k)) for k in range(7)]
    for kw in cases:
        rc, text = call(**kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_map_match"), (sorted(kw), rc, text)
    # legal and without work: batch 0 - nothing is enqueued, with or without buffers
    assert call(batch=0) == 0 and call(batch=0, state=None, poses=None, ws=None, ws_bytes=0) == 0
    assert all((b == 0x5A).all() for b in bufs.values())
    for bad in (dict(bytes=None), dict(frame=None), dict(frame=bad_frames[0]), dict(batch=-1), dict(batch=65536), dict(w_free=-1), dict(w_free=32768)):
        a = dict(dict(frame=frame, batch=1, w_free=0, bytes=need), **bad)
        before = need.value
        rc = L.sv_map_match_workspace(None if a["frame"] is None else ctypes.byref(a["frame"]), a["batch"], a["w_free"], None if a["bytes"] is None else ctypes.byref(a["bytes"]))
        assert rc == SV_ERR_ARG and need.value == before and L.sv_last_error(None).startswith(b"sv_map_match_workspace"), bad
    assert eng.debug_map_match(0, None) == 0
    for bad in (-1, 3, 512):
        assert eng.debug_map_match(bad, None) == SV_ERR_ARG
    assert eng.debug_map_match(0, None) == 0


def test_header_build_and_loader_agree(eng):
    """The library exports the entries the header declares for group (L), none of them an `occupancy` name, and build.py lists the new sources
    and header."""
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z_]*map_match[a-z_]*)\s*\(", src))
    assert declared == {"sv_map_match_workspace", "sv_map_match_device", "sv_debug_map_match"}
    L = eng.map_match_lib()
    assert all(hasattr(L, n) for n in declared) and len(L.sv_map_match_device.argtypes) == 16 and len(L.sv_map_match_workspace.argtypes) == 4
    build = util.pkg("build")
    assert "map_match_kernels.hip" in build.SOURCES and "map_match.cpp" in build.SOURCES and "map_match_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("map_match_kernels.hip", "map_match.cpp", "map_match_kernels.h"))
    mc.check_map_cells(build)  # the cell rules the map's readers share are defined once
    sv_mod = util.pkg("stereo_vision.sv")
    assert "occupancy_match" in sv_mod.__doc__ and "occupancy_pose_window" in sv_mod.__doc__ and "(L)" in text and "sgn(kx)" in text


def _results(res):
    out = {k: getattr(res, k).cpu().numpy() for k in ("sums", "counts", "best", "best_score")}
    return out


def test_map_class_matches_and_localizes_on_cpu_tensors(sv):
    """rig.OccupancyMap.match / localize on CPU tensors run the numpy definition: the host logic without a GPU."""
    import torch
    rigmod = util.pkg("rig")
    state = _recovery_state()
    world = rigmod.OccupancyMap(device="cpu", **RECOVERY_MAP)
    world.update(torch.from_numpy(state), sv.occupancy_pose(3.25, -1.5, 0.3)[None], RECOVERY_FRAME)
    before = world.logodds.clone()
    window = sv.occupancy_pose_window(3.0, -1.0, 0.3, *RECOVERY_WINDOW)
    poses = sv.occupancy_pose(window[:, 0], window[:, 1], window[:, 2])
    want = sv.occupancy_match(state, poses, RECOVERY_FRAME, world.words, world.logodds.numpy(), 2, 1)
    for given in (poses[None], torch.from_numpy(poses[None])):
        res = world.match(torch.from_numpy(state[None]), given, RECOVERY_FRAME, w_occ=2, w_free=1)
        assert isinstance(res, util.pkg("engine").MapMatchResult) and all(_bits(v, want[k]) for k, v in _results(res).items())
        assert _bits(res.score(2, 1).numpy(), want["score"])
    xyyaw, res = world.localize(state, (3.0, -1.0, 0.3), *RECOVERY_WINDOW, frame_grid=RECOVERY_FRAME, w_occ=2, w_free=1)
    assert xyyaw.shape == (1, 3) and xyyaw[0].tolist() == [3.25, -1.5, 0.3] and _bits(res.best.numpy(), want["best"])
    # two frames, each with its own guess; the map is left as it was
    both, _ = world.localize(np.stack([state, state]), [(3.0, -1.0, 0.3), (3.25, -1.5, 0.3)], *RECOVERY_WINDOW, frame_grid=RECOVERY_FRAME)
    assert both.tolist() == [[3.25, -1.5, 0.3]] * 2 and torch.equal(world.logodds, before) and world.seq == 1
    with pytest.raises(ValueError):
        world.match(torch.from_numpy(state[None]), poses[None])  # no frame grid
    with pytest.raises(ValueError):
        world.localize(state, [(0, 0, 0)] * 2, *RECOVERY_WINDOW, frame_grid=RECOVERY_FRAME)
    with pytest.raises(ValueError):
        world.match(torch.from_numpy(state[None]), poses[None], RECOVERY_FRAME, w_occ=0)


# ---------------------------------------------------------------------------------------------------------------- GPU

SMALL_MAPS = {"plain": dict(top=120, left=80),        # x -10..30, y -20..20 at scale 4: the recovery scene's
              "negative": dict(top=-37, left=-5)}      # wholly in negative x and y
LIST_SIZES = (0, 1, 63, 64, 65, 257, 2401)             # every wavefront and workgroup edge of the list, and past one staged chunk of 1024


def _small_words(sv, name):
    return sv.occupancy_map_words(dict(dict(rows=160, cols=160, scale=4, l_occ=85, l_free=40, l_min=-200, l_max=350), **SMALL_MAPS[name]))


def _state_with(rng, n_occ, n_free):
    """49 x 49 with exactly these numbers of state-2 and state-1 cells at random places; the rest 0, 3 and 255."""
    st = rng.choice(np.array([0, 3, 255], np.uint8), 2401)
    where = rng.permutation(2401)
    st[where[:n_occ]] = 2
    st[where[n_occ:n_occ + n_free]] = 1
    return st.reshape(49, 49)


def _poses_around(sv, rng, words, n):
    """n poses: a window that keeps the frame inside the map, then - as far as n allows - poses that clip it against each of the four edges,
    poses that miss the map and poses with words that are not finite."""
    ms = float(words["scale"])
    cx, cy = (words["top"] - words["rows"] / 2) / ms, (words["left"] - words["cols"] / 2) / ms  # the map's middle
    yaw = rng.uniform(-3.1, 3.1, n)
    x, y = cx - 6.0 * np.cos(yaw) + rng.uniform(-3, 3, n), cy - 6.0 * np.sin(yaw) + rng.uniform(-3, 3, n)  # the frame's middle (6, 0) near the map's
    p = sv.occupancy_pose(x, y, yaw)
    special = [(cx + 16.0, cy, 1.0, 0.0), (cx - 26.0, cy, 1.0, 0.0), (cx - 6.0, cy + 18.0, 1.0, 0.0), (cx - 6.0, cy - 18.5, 1.0, 0.0), (cx, cy - 27.0, 0.0, 1.0),
               (cx + 1000.0, cy, 1.0, 0.0), (NAN, cy, 1.0, 0.0), (cx, INF, 1.0, 0.0), (cx, cy, NAN, 0.0), (cx, cy, 1.0, -INF), (1e300, -1e300, 0.6, 0.8)]
    for k, pose in enumerate(special[:max(n - 1, 0)]):
        p[n - 1 - k] = pose
    return p


def _gpu(eng, state, poses, frame, words, logodds, w_occ=1, w_free=0):
    """engine.occupancy_match on numpy arrays -> dict of numpy arrays, the score from the sums."""
    res = eng.occupancy_match(_cuda(np.asarray(state, np.uint8)), np.asarray(poses, np.float64), frame, words, _cuda(logodds), w_occ, w_free)
    out = _results(res)
    out["score"] = res.score(w_occ, w_free).cpu().numpy()
    return out


def _counted(eng, group, fn):
    """fn() under sv_debug_map_match(group, counter) -> (its result, the lookups counted)."""
    import torch
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        assert eng.debug_map_match(group, counter) == 0
        out = fn()
        torch.cuda.synchronize()
    finally:
        eng.debug_map_match(0, None)
    return out, int(counter.item())


@pytest.mark.gpu
@pytest.mark.parametrize("n_poses", [1, 63, 64, 65, 245, 300])
@pytest.mark.parametrize("map_name", sorted(SMALL_MAPS))
def test_smallest_shapes_equal_the_definition(sv, eng, map_name, n_poses):
    """Batch 3 with an empty frame in the middle, lists of every size at which the kernels take another path, all the ways a workgroup may
    be shared out among candidates, free cells off and on, the whole int16 range in the map."""
    words = _small_words(sv, map_name)
    rng = np.random.default_rng(100 + n_poses)
    logodds = rng.integers(-32768, 32768, (160, 160)).astype(np.int16)
    logodds[rng.integers(0, 160, 300), rng.integers(0, 160, 300)] = -32768
    logodds[rng.integers(0, 160, 300), rng.integers(0, 160, 300)] = 32767
    poses = np.stack([_poses_around(sv, rng, words, n_poses) for _ in range(3)])
    clipped = False
    for n in LIST_SIZES:
        state = np.stack([_state_with(rng, n, min(n, 2401 - n)), rng.choice(np.array([0, 3, 77], np.uint8), (49, 49)), _state_with(rng, 700, 900)])
        for w_occ, w_free in ((1, 0), (3, 2)):
            want = sv.occupancy_match(state, poses, RECOVERY_FRAME, words, logodds, w_occ, w_free)
            assert not want["sums"][1].any() and want["best"][1] == 0
            full = (n, 0 if w_free == 0 else min(n, 2401 - n))
            clipped |= n == 257 and n_poses >= 6 and (0 < want["counts"][0, -5:, 0]).all() and (want["counts"][0, -5:, 0] < 257).all()
            assert n_poses < 12 or n == 0 or (want["counts"][0, :-11] == full).all() and not want["counts"][0, -11:-5].any()
            per_list = (n + full[1] + 0 + (700 + (900 if w_free else 0))) * n_poses
            for group in (0, 1, 8, 64, 256):
                got, lookups = _counted(eng, group, lambda: _gpu(eng, state, poses, RECOVERY_FRAME, words, logodds, w_occ, w_free))
                assert _same(got, want), (map_name, n_poses, n, w_free, group, [k for k in KEYS if not _bits(got[k], want[k])])
                assert lookups == per_list, (n, w_free, group)
    assert clipped or n_poses < 6  # the four edges each cut some of the frame's cells off, none all of them


def _raw(eng, state, poses, frame, spec, logodds, w_occ, w_free, sums, counts, best, best_score, ws, stream=None):
    """The C entry on caller-owned tensors."""
    import torch
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    return eng.map_match_lib().sv_map_match_device(ptr(state), ptr(poses), state.shape[0], poses.shape[1], ctypes.byref(frame), ctypes.byref(spec), ptr(logodds), w_occ, w_free,
                                                   ptr(sums), ptr(counts), ptr(best), ptr(best_score), ptr(ws), 0 if ws is None else ws.numel() * ws.element_size(),
                                                   (torch.cuda.current_stream() if stream is None else stream).cuda_stream)


@pytest.mark.gpu
def test_buffer_use_streams_and_refusals(sv, eng):
    """Pre-filled outputs and a dirty workspace, either pair of outputs left out, repeats, a stream of its own, a map after a recenter; and the
    C entry's refusals on device buffers, which stay as they were."""
    import torch
    rigmod = util.pkg("rig")
    rng = np.random.default_rng(41)
    world = rigmod.OccupancyMap(**RECOVERY_MAP)
    cpu = rigmod.OccupancyMap(device="cpu", **RECOVERY_MAP)
    L0 = rng.integers(-32768, 32768, (160, 160)).astype(np.int16)
    world.logodds.copy_(_cuda(L0))
    cpu.logodds.copy_(torch.from_numpy(L0))
    assert world.recenter(17.3, -8.6) == cpu.recenter(17.3, -8.6) != (0, 0) and world.words == cpu.words and world.words["top"] != 120
    words = world.words
    state = np.stack([_state_with(rng, 300, 1500), _state_with(rng, 0, 0), _state_with(rng, 1100, 1301)])
    poses = np.stack([_poses_around(sv, rng, words, 70) for _ in range(3)])
    want = sv.occupancy_match(state, poses, RECOVERY_FRAME, words, cpu.logodds.numpy(), 5, 7)
    assert want["counts"].any() and (want["counts"][1] == 0).all()
    frame, spec = eng.occupancy_spec(z_range=(-1, 1), **RECOVERY_FRAME)[0], eng._occupancy_map_struct(words)
    need = ctypes.c_size_t()
    assert eng.map_match_lib().sv_map_match_workspace(ctypes.byref(frame), 3, 7, ctypes.byref(need)) == 0
    t_state, t_poses = _cuda(state), _cuda(poses)

    def outputs():
        return (torch.full((3, 70, 2), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda"), torch.full((3, 70, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda"),
                torch.full((3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda"), torch.full((3,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda"))

    side = torch.cuda.Stream()
    ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda")
    seen = set()
    for rep, stream in enumerate((None, None, side, side, None)):
        sums, counts, best, best_score = outputs()
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        assert _raw(eng, t_state, t_poses, frame, spec, world.logodds, 5, 7, sums, counts, best, best_score, ws, stream) == 0
        if stream is not None:
            torch.cuda.current_stream().wait_stream(stream)
        got = dict(sums=sums.cpu().numpy(), counts=counts.cpu().numpy(), best=best.cpu().numpy(), best_score=best_score.cpu().numpy())
        assert all(_bits(got[k], want[k]) for k in got), rep
        seen.add(b"".join(got[k].tobytes() for k in sorted(got)))
    assert len(seen) == 1
    # only the best, only the sums: what is not asked for is not written
    sums, counts, best, best_score = outputs()
    assert _raw(eng, t_state, t_poses, frame, spec, world.logodds, 5, 7, None, None, best, best_score, ws) == 0
    assert _bits(best.cpu().numpy(), want["best"]) and _bits(best_score.cpu().numpy(), want["best_score"]) and (sums == 0x5A5A5A5A5A5A5A5A).all() and (counts == 0x5A5A5A5A).all()
    sums, counts, best, best_score = outputs()
    assert _raw(eng, t_state, t_poses, frame, spec, world.logodds, 5, 7, sums, counts, None, None, ws) == 0
    assert _bits(sums.cpu().numpy(), want["sums"]) and _bits(counts.cpu().numpy(), want["counts"]) and (best == 0x5A5A5A5A).all() and (best_score == 0x5A5A5A5A5A5A5A5A).all()
    res = eng.occupancy_match(t_state, t_poses, RECOVERY_FRAME, words, world.logodds, 5, 7, want_sums=False)
    assert res.sums is None and res.counts is None and _bits(res.best.cpu().numpy(), want["best"])
    # refused on the device as on the host: nothing is written
    sums, counts, best, best_score = outputs()
    small = torch.empty(need.value - 16, dtype=torch.uint8, device="cuda")
    for kw in (dict(ws=small), dict(ws=None), dict(w_occ=0, w_free=0), dict(w_free=32768), dict(counts=None), dict(best=None), dict(logodds=None)):
        a = dict(dict(state=t_state, poses=t_poses, frame=frame, spec=spec, logodds=world.logodds, w_occ=5, w_free=7, sums=sums, counts=counts, best=best, best_score=best_score, ws=ws), **kw)
        assert _raw(eng, **a) == SV_ERR_ARG and eng.map_match_lib().sv_last_error(None).startswith(b"sv_map_match"), sorted(kw)
    torch.cuda.synchronize()
    assert (sums == 0x5A5A5A5A5A5A5A5A).all() and (counts == 0x5A5A5A5A).all() and (best == 0x5A5A5A5A).all() and (best_score == 0x5A5A5A5A5A5A5A5A).all()
    for bad in (dict(state=t_state.int()), dict(state=t_state.cpu()), dict(poses=poses[:2]), dict(poses=t_poses.float()), dict(logodds=world.logodds.int()), dict(w_occ=0),
                dict(w_free=-1), dict(map=dict(words, rows=0)), dict(frame_grid=dict(RECOVERY_FRAME, scale=0)), dict(want_sums=False, want_best=False)):
        with pytest.raises(ValueError):
            eng.occupancy_match(**dict(dict(state=t_state, poses=poses, frame_grid=RECOVERY_FRAME, map=words, logodds=world.logodds), **bad))
    # rig.OccupancyMap on the device against the class on CPU tensors
    res, res_cpu = world.match(t_state, poses, RECOVERY_FRAME, 5, 7), cpu.match(state, poses, RECOVERY_FRAME, 5, 7)
    assert all(_bits(getattr(res, k).cpu().numpy(), getattr(res_cpu, k).numpy()) for k in ("sums", "counts", "best", "best_score"))
    assert eng.occupancy_match(t_state[:0], np.zeros((0, 5, 4)), RECOVERY_FRAME, words, world.logodds).best.shape == (0,)


@pytest.mark.gpu
def test_the_committed_drive(sv, eng, drive):
    """The seven KITTI frames fused along their poses, then each matched over a 5 x 5 x 3 window around its pose: the C entry through the
    engine, rig.OccupancyMap.match and localize, and the class on CPU tensors."""
    import torch
    occ, states, poses, words, fused = drive
    rigmod = util.pkg("rig")
    xyyaw = np.stack([0.8 * np.arange(7.0), 0.05 * np.arange(7.0), 0.03 * np.arange(7.0)], -1)
    half, steps = (0.2, 0.2, 0.01), (5, 5, 3)
    window = np.stack([sv.occupancy_pose_window(x, y, yaw, half, steps) for x, y, yaw in xyyaw])
    cand = sv.occupancy_pose(window[..., 0], window[..., 1], window[..., 2])
    assert cand.shape == (7, 75, 4)
    logodds = _cuda(fused["logodds"])
    for w_free in (0, 1):
        want = sv.occupancy_match(states, cand, CLI_GRID, words, fused["logodds"], 1, w_free)
        (got, lookups) = _counted(eng, 0, lambda: eng.occupancy_match(occ.state, cand, occ.spec, words, logodds, 1, w_free))
        got = dict(_results(got), score=got.score(1, w_free).cpu().numpy())
        assert _same(got, want), w_free
        assert lookups == 75 * (int((states == 2).sum()) + (int((states == 1).sum()) if w_free else 0))
        # the map covers every window: each frame's occupied cells all land in it, under every candidate
        assert (want["counts"][..., 0] == (states == 2).sum((1, 2))[:, None]).all() and want["sums"][..., 0].any()
        print("w_free %d: best %s of 75, lookups %d" % (w_free, want["best"].tolist(), lookups))
    world, cpu = rigmod.OccupancyMap(**DRIVE_MAP), rigmod.OccupancyMap(device="cpu", **DRIVE_MAP)
    world.logodds.copy_(logodds)
    cpu.logodds.copy_(torch.from_numpy(fused["logodds"]))
    refined, res = world.localize(occ, xyyaw, half, steps, w_free=1)
    refined_cpu, res_cpu = cpu.localize(states, xyyaw, half, steps, frame_grid=CLI_GRID, w_free=1)
    assert _bits(refined, refined_cpu) and _bits(res.best.cpu().numpy(), want["best"]) and _bits(res_cpu.sums.numpy(), want["sums"])
    assert _bits(refined, window[np.arange(7), want["best"]])


@pytest.mark.gpu
def test_cli_matches_before_it_fuses(sv, eng, drive, tmp_path):
    from PIL import Image
    occ, states, _, _, _ = drive
    n = 2
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    ls, rs = _drive_frames(n)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    guesses = np.array([[0.0, 0.0, 0.0], [0.9, 0.1, 0.02]])
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("".join("%r %r %r\n" % tuple(float(v) for v in row) for row in guesses))
    out = str(tmp_path / "map.png")
    common = ["-k", str(tmp_path / "kitti"), "--batch", "2"]
    for bad in (["--match", "0.2,0.2,0.01"], ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--match", "0.2,0.2"],
                ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--match", "0.2,0.2,0.01,2,3,3"],
                ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--match", "0.2,-0.2,0.01"],
                ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--match", "a,b,c"]):
        with pytest.raises(SystemExit):
            sv.main(common + bad)
    assert not os.path.exists(out)
    sv.main(common + ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--match", "0.2,0.2,0.01,5,5,3"])
    ranges = sv.occupancy_map_cover(guesses, sv.CLI_TOP_VIEW["x_range"], sv.CLI_TOP_VIEW["y_range"])
    cpu = util.pkg("rig").OccupancyMap(ranges[0], ranges[1], 10, device="cpu")
    cpu.update(states[:1], sv.occupancy_pose(*guesses[0])[None], CLI_GRID)
    refined, _ = cpu.localize(states[1:2], guesses[1], (0.2, 0.2, 0.01), (5, 5, 3), frame_grid=CLI_GRID)
    cpu.update(states[1:2], sv.occupancy_pose(*refined[0])[None], CLI_GRID)
    written = sv.read_poses(str(tmp_path / "map.poses.txt"), 2)
    assert _bits(written, np.stack([guesses[0], refined[0]]))
    got = np.asarray(Image.open(out))
    assert np.array_equal(got, sv.OCCUPANCY_PNG[cpu.state().numpy()]) and set(np.unique(got).tolist()) == {0, 127, 255}
    # without --match the same command fuses at the lines' poses and writes no poses file
    os.remove(tmp_path / "map.poses.txt")
    sv.main(common + ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt")])
    plain = util.pkg("rig").OccupancyMap(ranges[0], ranges[1], 10, device="cpu")
    plain.update(states[:2], sv.occupancy_pose(guesses[:, 0], guesses[:, 1], guesses[:, 2]), CLI_GRID)
    assert np.array_equal(np.asarray(Image.open(out)), sv.OCCUPANCY_PNG[plain.state().numpy()]) and not os.path.exists(tmp_path / "map.poses.txt")
