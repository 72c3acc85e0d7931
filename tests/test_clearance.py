"""The clearance field of the world map and the path check against it (include/stereo_vision_hip.h (M)): the numpy definitions in
stereo_vision.sv on hand-computed cases and against the all-pairs form, the cell rule against the correlative match, the argument checks in
Python and in the C ABI, and the HIP kernels - C entry, engine, rig.OccupancyMap.clearance / check_paths and the CLI's --clearance - against
the definitions.

Everything is compared exactly: equal shape, dtype and bits.  That is derived, not chosen: the field is a minimum of integers, which no
order or decomposition can change; the path check's only doubles - a disc centre carried into the world - are products, sums and
comparisons in a stated order (-ffp-contract=off on the device, numpy never fuses), and behind floor() it is two minima and a count."""
import ctypes
import os
import re

import numpy as np
import pytest

import map_stage_cases as mc
import util
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_occupancy_map import CLI_GRID, _drive_frames, drive  # noqa: F401 (drive: the committed KITTI frames' states, a fixture)
from test_map_match import HAND_MAP, RECOVERY_FRAME, RECOVERY_MAP, SMALL_MAPS, _BAD_MAPS, _c_map, _poses_around, _recovery_state, _small_words

SV_ERR_ARG = -1
NAN, INF = float("nan"), float("inf")
F = 65535
PATH_KEYS = ("first_hit", "min_d2", "n_outside")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- CPU

# 5 x 7 cells, sources at (1, 1) and (4, 6), R = 2: everything up to distance^2 4 is kept - (1, 3) and (3, 1) lie exactly R from the first
# source - and (2, 3), at 1 + 4 = 5 = R^2 + 1 from it, is saturated.
HAND_FIELD = np.array([[2, 1, 2, F, F, F, F],
                       [1, 0, 1, 4, F, F, F],
                       [2, 1, 2, F, F, F, 4],
                       [F, 4, F, F, F, 2, 1],
                       [F, F, F, F, 4, 1, 0]], np.uint16)


def test_hand_computed_field(sv):
    L = np.full((5, 7), -3, np.int16)
    L[1, 1], L[4, 6] = 90, 85
    for form in (sv.occupancy_clearance, sv.occupancy_clearance_brute):
        got = form(L, 2, 85)
        assert got.dtype == np.uint16 and got.tolist() == HAND_FIELD.tolist()
        # one more cell of radius lets the 5s and 8s in, nothing else: 9 = 3^2 is the bound
        wider = form(L, 3, 85)
        assert wider[2, 3] == 5 and wider[3, 3] == 8 and wider[1, 4] == 9 and wider[0, 4] == F and (wider[HAND_FIELD != F] == HAND_FIELD[HAND_FIELD != F]).all()
        # the threshold is >=; a never-seen cell is a source only when asked for
        assert form(L, 2, 86).tolist() == form(np.where(L == 85, -3, L).astype(np.int16), 2, 85).tolist() and form(L, 2, 91).min() == F
        S = np.zeros((5, 7), np.int32)
        S[4, 6] = -1
        assert form(L, 2, 86, S).tolist() == form(L, 2, 86).tolist() and form(L, 2, 86, S, True).tolist() == HAND_FIELD.tolist()
    # the map's edge is no obstacle
    assert sv.occupancy_clearance(np.zeros((3, 4), np.int16), 254, 1).tolist() == [[F] * 4] * 3


def _random_map(rng, rows, cols, density):
    """(logodds, last_seen, t_occ): about `density` of the cells at or above t_occ (exactly one for density "one"), a few never seen."""
    L = rng.integers(-200, 50, (rows, cols)).astype(np.int16)
    if density == "one":
        L[rng.integers(rows), rng.integers(cols)] = 99
    else:
        L[rng.random((rows, cols)) < density] = 99
    return L, rng.choice(np.array([-1, 0, 5], np.int32), (rows, cols), p=[0.02, 0.49, 0.49]), 85


def test_two_pass_form_equals_brute_force(sv):
    rng = np.random.default_rng(7)
    densities = [0.0, "one", 0.01, 0.5, 1.0]
    for k in range(30):
        rows, cols = (int(v) for v in rng.integers(1, 41, 2)) if k else (40, 40)
        L, S, t = _random_map(rng, rows, cols, densities[k % 5])
        for R in (1, 2, 7, 39, 254):
            for unknown in (False, True):
                for t_occ in (t, -32768, 32767):
                    a, b = sv.occupancy_clearance(L, R, t_occ, S, unknown), sv.occupancy_clearance_brute(L, R, t_occ, S, unknown)
                    assert _bits(a, b), (rows, cols, densities[k % 5], R, unknown, t_occ)
                    assert t_occ != -32768 or not a.any()  # everything is a source
                    assert ((a == 0) == ((L >= t_occ) | (unknown & (S < 0)))).all() and (a[a != F] <= R * R).all()
    try:  # where scipy is there: the exact Euclidean transform, squared and capped
        from scipy.ndimage import distance_transform_edt
    except ImportError:
        return
    L, S, t = _random_map(rng, 40, 33, 0.01)
    d = np.rint(distance_transform_edt(L < t) ** 2).astype(np.int64)
    assert _bits(sv.occupancy_clearance(L, 7, t), np.where(d > 49, F, d).astype(np.uint16))


# HAND_MAP: x 0..4, y -2..2 at scale 1; the world point (Xw, Yw) lies in cell (3 - floor(Xw), 1 - floor(Yw)).  The field of one source at
# (1, 3) with R = 2:
HAND_D2 = np.array([[F, F, 2, 1],
                    [F, 4, 1, 0],
                    [F, F, 2, 1],
                    [F, F, F, 4]], np.uint16)
# one disc at the vehicle's origin with r2 = 1, three steps per path, zero yaw:
#   clear    (0.5, 1.5) -> (3, 0) = F, (0.5, 0.5) -> (3, 1) = F, (2.5, 0.5) -> (1, 1) = 4 > 1: no hit, least 4
#   hit      (0.5, 1.5) -> F, (1.5, -0.5) -> (2, 2) = 2 > 1, (2.5, -0.5) -> (1, 2) = 1 <= 1: d2 == r2 is a hit, at step 2
#   leaves   (0.5, 0.5) -> (3, 1) = F, (-0.5, 0.5) has gx = -1 < top - rows, (4.0, 0.5) has gx = 4 > top - 1: two outside, least F
#   nan      tx = nan: outside; (2.5, -1.5) -> (1, 3) = 0: a hit at step 1; c = nan: outside
HAND_PATHS = [[(0.5, 1.5, 1.0, 0.0), (0.5, 0.5, 1.0, 0.0), (2.5, 0.5, 1.0, 0.0)],
              [(0.5, 1.5, 1.0, 0.0), (1.5, -0.5, 1.0, 0.0), (2.5, -0.5, 1.0, 0.0)],
              [(0.5, 0.5, 1.0, 0.0), (-0.5, 0.5, 1.0, 0.0), (4.0, 0.5, 1.0, 0.0)],
              [(NAN, 0.5, 1.0, 0.0), (2.5, -1.5, 1.0, 0.0), (0.5, 0.5, NAN, 0.0)]]
HAND_PATH_RESULT = dict(first_hit=[3, 2, 3, 1], min_d2=[4, 1, F, 0], n_outside=[0, 0, 2, 2])


def test_hand_computed_path_check(sv):
    L = np.zeros((4, 4), np.int16)
    L[1, 3] = 85
    assert sv.occupancy_clearance(L, 2, 85).tolist() == HAND_D2.tolist()
    got = sv.clearance_paths(HAND_D2, HAND_MAP, HAND_PATHS, [(0.0, 0.0)], np.array([1], np.int32), 2)
    assert all(got[k].dtype == np.int32 and got[k].tolist() == HAND_PATH_RESULT[k] for k in PATH_KEYS), got
    # r2 = 0 touches only a source: the second path is clear now, the fourth still stands on one
    got = sv.clearance_paths(HAND_D2, HAND_MAP, HAND_PATHS, [(0.0, 0.0)], np.array([0], np.int32), 2)
    assert got["first_hit"].tolist() == [3, 3, 3, 1] and got["min_d2"].tolist() == HAND_PATH_RESULT["min_d2"]
    # two discs, the second one metre ahead with r2 = R^2: at (1.5, -1.5) turned a quarter (c, s) = (0, 1) it lies at (1.5, -0.5) ->
    # (2, 2) = 2 <= 4, the first at (1.5, -1.5) -> (2, 3) = 1 > 0; not turned it lies at (2.5, -1.5) -> (1, 3) = 0; at (3.5, 1.5) it
    # has left the map and the first stands on (0, 0) = F
    paths = [[(1.5, -1.5, 0.0, 1.0)], [(1.5, -1.5, 1.0, 0.0)], [(3.5, 1.5, 1.0, 0.0)]]
    got = sv.clearance_paths(HAND_D2, HAND_MAP, paths, [(0.0, 0.0), (1.0, 0.0)], np.array([0, 4], np.int32), 2)
    assert got["first_hit"].tolist() == [0, 0, 1] and got["min_d2"].tolist() == [1, 0, F] and got["n_outside"].tolist() == [0, 0, 1]
    centres, r2 = sv.clearance_discs([(0.0, 0.0, 0.0), (1.0, 0.0, 0.11), (-0.5, 0.25, 0.3)], 10)
    assert centres.dtype == np.float64 and centres.tolist() == [[0.0, 0.0], [1.0, 0.0], [-0.5, 0.25]] and r2.dtype == np.int32 and r2.tolist() == [0, 4, 9]
    assert sv.clearance_png(np.array([[0, 1, 3, 4], [8, 9, 64516, F]], np.uint16)).tolist() == [[0, 1, 1, 2], [2, 3, 254, 255]]


def test_cell_rule_is_the_match_s(sv):
    """A frame with one occupied cell scored against a map whose log-odds name their cell, and a disc at that cell's point looked up in a
    field whose values name theirs: the same cell under every pose, and outside under the same poses."""
    words = _small_words(sv, "negative")
    at = np.arange(160 * 160, dtype=np.int64).reshape(160, 160)
    logodds, d2 = (at - 12800).astype(np.int16), at.astype(np.uint16)
    Xf, Yf = sv.occupancy_frame_points(RECOVERY_FRAME)
    rng = np.random.default_rng(11)
    poses = _poses_around(sv, rng, words, 400)
    for fr, fc in ((5, 10), (48, 24), (20, 47), (24, 0)):
        state = np.zeros((49, 49), np.uint8)
        state[fr, fc] = 2
        match = sv.occupancy_match(state, poses, RECOVERY_FRAME, words, logodds)
        got = sv.clearance_paths(d2, words, poses[:, None, :], [(Xf[fr], Yf[fc])], np.array([0], np.int32), 1)
        inside = match["counts"][0, :, 0] == 1
        assert 300 < inside.sum() < 400 and _bits(got["n_outside"], (1 - match["counts"][0, :, 0]).astype(np.int32))
        assert (got["min_d2"][inside] - 12800 == match["sums"][0, inside, 0]).all() and (got["min_d2"][~inside] == F).all()
        ok, r, c = sv.clearance_cells(words, poses, [(Xf[fr], Yf[fc])])
        assert _bits(ok[:, 0], inside) and (at[r[inside, 0], c[inside, 0]] == got["min_d2"][inside]).all()


def _c_paths_call(L, base, **kw):
    a = dict(base, **kw)
    return L.sv_clearance_paths_device(a["d2"], None if a["map"] is None else ctypes.byref(a["map"]), a["poses"], a["n_paths"], a["n_steps"], a["centres"], a["r2"],
                                       a["n_discs"], a["radius"], a["first_hit"], a["min_d2"], a["n_outside"], a["stream"])


def _c_field_call(L, base, **kw):
    a = dict(base, **kw)
    return L.sv_clearance_device(a["logodds"], a["last_seen"], a["rows"], a["cols"], a["radius"], a["t_occ"], a["unknown"], a["d2"], a["ws"], a["ws_bytes"], a["stream"])


_BAD_FIELD = [dict(rows=0), dict(cols=0), dict(rows=32769), dict(cols=-1), dict(radius=0), dict(radius=255), dict(radius=-1), dict(t_occ=32768), dict(t_occ=-32769),
              dict(unknown=2), dict(unknown=-1)]
_BAD_PATHS = [dict(n_paths=-1), dict(n_paths=65536), dict(n_steps=0), dict(n_steps=65536), dict(n_discs=0), dict(n_discs=65), dict(radius=0), dict(radius=255)]


def test_validation_needs_no_device(sv, eng):
    """Every refused argument raises ValueError in Python; the C entries return SV_ERR_ARG on host buffers, which stay untouched: the checks
    run before any HIP call."""
    L16, S32 = np.zeros((4, 6), np.int16), np.zeros((4, 6), np.int32)
    for bad in (dict(radius=0), dict(radius=255), dict(radius=1.5), dict(radius=True), dict(t_occ=32768), dict(t_occ=-32769), dict(t_occ=0.5), dict(unknown=2),
                dict(unknown=True, last_seen=None), dict(logodds=L16.astype(np.int32)), dict(logodds=L16[0]), dict(last_seen=S32[:3]), dict(last_seen=S32.astype(np.int64))):
        for form in (sv.occupancy_clearance, sv.occupancy_clearance_brute):
            with pytest.raises(ValueError):
                form(**dict(dict(logodds=L16, radius=2, t_occ=1, last_seen=S32, unknown=False), **bad))
    good = dict(d2=HAND_D2, map=HAND_MAP, poses=HAND_PATHS, centres=[(0.0, 0.0)], r2=np.array([4], np.int32), radius=2)
    for bad in [dict(map=dict(HAND_MAP, **kw)) for kw in _BAD_MAPS] + [dict(r2=np.array([5], np.int32)), dict(r2=np.array([-1], np.int32)), dict(r2=np.array([1.0])),
                                                                        dict(r2=np.array([1, 1], np.int32)), dict(centres=[(0.0, 0.0, 0.0)]), dict(centres=np.zeros((65, 2)), r2=np.zeros(65, np.int32)),
                                                                        dict(centres=np.zeros((0, 2)), r2=np.zeros(0, np.int32)), dict(radius=0), dict(radius=255), dict(d2=HAND_D2.astype(np.int32)),
                                                                        dict(d2=HAND_D2[:3]), dict(poses=np.zeros((2, 3, 3))), dict(poses=np.zeros((2, 0, 4))), dict(poses=np.zeros((3, 4)))]:
        with pytest.raises(ValueError):
            sv.clearance_paths(**dict(good, **bad))
    for bad in (dict(discs_m=[(0, 0)]), dict(discs_m=[(0, 0, -1)]), dict(discs_m=[(NAN, 0, 1)]), dict(discs_m=np.zeros((65, 3))), dict(discs_m=[(0, 0, 25.5)]), dict(scale=0),
                dict(scale=2.5)):
        with pytest.raises(ValueError):
            sv.clearance_discs(**dict(dict(discs_m=[(0, 0, 1)], scale=10), **bad))

    L = eng.clearance_lib()
    need = ctypes.c_size_t(0)
    assert L.sv_clearance_workspace(4, 6, ctypes.byref(need)) == 0 and need.value == 32
    assert L.sv_clearance_workspace(32768, 32768, ctypes.byref(need)) == 0 and need.value == 2 ** 30
    assert L.sv_clearance_workspace(1, 1, ctypes.byref(need)) == 0 and need.value == 16
    for rows, cols, out in ((0, 1, need), (1, 0, need), (32769, 1, need), (1, 40000, need), (-1, 1, need), (4, 6, None)):
        assert L.sv_clearance_workspace(rows, cols, None if out is None else ctypes.byref(out)) == SV_ERR_ARG and need.value == 16
        assert L.sv_last_error(None).startswith(b"sv_clearance_workspace")
    bufs = {k: np.full(256, 0x5A, np.uint8) for k in ("logodds", "last_seen", "d2", "ws", "poses", "first_hit", "min_d2", "n_outside")}
    ptr = lambda name: bufs[name].ctypes.data + (-bufs[name].ctypes.data) % 16  # noqa: E731
    base = dict(logodds=ptr("logodds"), last_seen=ptr("last_seen"), rows=4, cols=6, radius=2, t_occ=85, unknown=1, d2=ptr("d2"), ws=ptr("ws"), ws_bytes=32, stream=None)
    cases = _BAD_FIELD + [dict(logodds=None), dict(d2=None), dict(ws=None), dict(last_seen=None), dict(logodds=ptr("logodds") + 1), dict(last_seen=ptr("last_seen") + 2),
                          dict(d2=ptr("d2") + 1), dict(ws=ptr("ws") + 8), dict(ws_bytes=31), dict(ws_bytes=0), dict(d2=ptr("logodds")), dict(d2=ptr("logodds") + 46),
                          dict(d2=ptr("last_seen") + 94), dict(d2=ptr("ws") + 30), dict(ws=ptr("d2") + 32), dict(rows=32768, cols=32768, ws_bytes=2 ** 30 - 16)]
    for kw in cases:
        rc, text = _c_field_call(L, base, **kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_clearance:"), (sorted(kw), rc, text)
    centres, r2 = np.array([[0.0, 0.0], [1.0, 0.5]]), np.array([0, 4], np.int32)
    pbase = dict(d2=ptr("d2"), map=_c_map(eng), poses=ptr("poses"), n_paths=2, n_steps=3, centres=centres.ctypes.data, r2=r2.ctypes.data, n_discs=2, radius=2,
                 first_hit=ptr("first_hit"), min_d2=ptr("min_d2"), n_outside=ptr("n_outside"), stream=None)
    low, neg = np.array([0, 5], np.int32), np.array([-1, 4], np.int32)
    cases = _BAD_PATHS + [dict(map=None), dict(d2=None), dict(poses=None), dict(centres=None), dict(r2=None), dict(first_hit=None), dict(min_d2=None), dict(n_outside=None),
                          dict(d2=ptr("d2") + 1), dict(poses=ptr("poses") + 4), dict(centres=centres.ctypes.data + 4), dict(r2=r2.ctypes.data + 2), dict(first_hit=ptr("first_hit") + 2),
                          dict(min_d2=ptr("min_d2") + 1), dict(n_outside=ptr("n_outside") + 2), dict(r2=low.ctypes.data), dict(r2=neg.ctypes.data), dict(radius=1)]
    cases += [dict(map=_c_map(eng, **kw)) for kw in _BAD_MAPS] + [dict(map=_c_map(eng, reserved=k)) for k in range(7)]
    for kw in cases:
        rc, text = _c_paths_call(L, pbase, **kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_clearance_paths"), (sorted(kw), rc, text)
    # legal and without work: no path - nothing is enqueued, with or without buffers
    assert _c_paths_call(L, pbase, n_paths=0) == 0 and _c_paths_call(L, pbase, n_paths=0, poses=None, first_hit=None, min_d2=None, n_outside=None) == 0
    assert all((b == 0x5A).all() for b in bufs.values())
    assert eng.debug_clearance(0, None) == 0
    for bad in (-1, 4, 17):
        assert eng.debug_clearance(bad, None) == SV_ERR_ARG and L.sv_last_error(None).startswith(b"sv_debug_clearance")
    assert eng.debug_clearance(0, None) == 0


def test_header_build_and_loader_agree(eng):
    """The library exports the four entries the header declares for group (M), none of them an `occupancy` or `map_match` name, and build.py
    lists the new sources and header."""
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z_]*clearance[a-z_]*)\s*\(", src))
    assert declared == {"sv_clearance_workspace", "sv_clearance_device", "sv_clearance_paths_device", "sv_debug_clearance"}
    L = eng.clearance_lib()
    assert all(hasattr(L, n) for n in declared)
    assert len(L.sv_clearance_device.argtypes) == 11 and len(L.sv_clearance_paths_device.argtypes) == 13 and len(L.sv_clearance_workspace.argtypes) == 3
    build = util.pkg("build")
    assert "clearance_kernels.hip" in build.SOURCES and "clearance.cpp" in build.SOURCES and "clearance_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("clearance_kernels.hip", "clearance.cpp", "clearance_kernels.h"))
    mc.check_map_cells(build)  # the cell rules the map's readers share are defined once
    sv_mod = util.pkg("stereo_vision.sv")
    assert all(n in sv_mod.__doc__ for n in ("occupancy_clearance", "occupancy_clearance_brute", "clearance_paths", "clearance_discs")) and "(M)" in text


def _fused_recovery_maps(sv, devices):
    rigmod = util.pkg("rig")
    maps = [rigmod.OccupancyMap(device=d, **RECOVERY_MAP) for d in devices]
    for m in maps:
        m.update(_recovery_state()[None], sv.occupancy_pose(3.25, -1.5, 0.3)[None], RECOVERY_FRAME)
    return maps


def _fan(sv, n_paths=12, n_steps=20):
    """(x, y, yaw) float64 [n_paths, n_steps, 3]: arcs from the recovery scene's vehicle pose, some through its walls, the widest off the map."""
    s = np.linspace(0.0, 1.0, n_steps)[None, :]
    bend = np.linspace(-1.2, 1.2, n_paths)[:, None]
    yaw = 0.3 + bend * s
    reach = np.linspace(6.0, 40.0, n_paths)[:, None]
    return np.stack([3.25 + reach * s * np.cos(yaw), -1.5 + reach * s * np.sin(yaw), yaw], -1)


FOOTPRINT_M = [(0.0, 0.0, 0.5), (1.0, 0.0, 0.5), (2.0, 0.0, 0.3)]


def test_map_class_on_cpu_tensors(sv):
    """rig.OccupancyMap.clearance / check_paths on CPU tensors run the numpy definitions: the host logic without a GPU."""
    import torch
    (world,) = _fused_recovery_maps(sv, ["cpu"])
    with pytest.raises(ValueError):
        world.check_paths(_fan(sv), FOOTPRINT_M)  # no field yet
    d2 = world.clearance(1.0)
    assert world.clearance_radius == 4 and d2.dtype == torch.uint16 and d2.device.type == "cpu"
    want = sv.occupancy_clearance(world.logodds.numpy(), 4, 85)
    assert _bits(d2.numpy(), want) and (want == 0).sum() == (world.logodds.numpy() >= 85).sum() > 50 and (want == F).any()
    assert world.clearance(0.76).shape == (160, 160) and world.clearance_radius == 4 and world.clearance(0.75) is not None and world.clearance_radius == 3
    assert _bits(world.clearance(1.0, occupied=-40, unknown=True).numpy(), sv.occupancy_clearance(world.logodds.numpy(), 4, -40, world.last_seen.numpy(), True))
    assert _bits(world.clearance(1.0).numpy(), want)
    for bad in (63.6, 0.0, -1.0, NAN, INF):  # 63.6 m are 255 cells
        with pytest.raises(ValueError):
            world.clearance(bad)
    assert world.clearance(63.5).shape == (160, 160) and world.clearance_radius == 254
    world.clearance(1.0)
    fan = _fan(sv)
    centres, r2 = sv.clearance_discs(FOOTPRINT_M, 4)
    assert r2.tolist() == [4, 4, 4]
    poses = sv.occupancy_pose(fan[..., 0], fan[..., 1], fan[..., 2])
    ref = sv.clearance_paths(want, world.words, poses, centres, r2, 4)
    assert (ref["first_hit"] < 20).any() and len(set(ref["first_hit"].tolist())) > 3 and ref["n_outside"].any() and not ref["n_outside"].all()
    for given in (fan, torch.from_numpy(fan), poses, torch.from_numpy(poses)):
        res = world.check_paths(given, FOOTPRINT_M)
        assert isinstance(res, util.pkg("engine").ClearancePathsResult) and all(_bits(getattr(res, k).numpy(), ref[k]) for k in PATH_KEYS)
    other = torch.from_numpy(np.full((160, 160), F, np.uint16))
    assert (world.check_paths(fan, FOOTPRINT_M, d2=other).first_hit == 20).all()
    for bad in (dict(paths=fan[0]), dict(paths=fan[..., :2]), dict(discs_m=[(0.0, 0.0, 1.01)]), dict(discs_m=[(0.0, 0.0)])):  # 1.01 m are 5 cells > R
        with pytest.raises(ValueError):
            world.check_paths(**dict(dict(paths=fan, discs_m=FOOTPRINT_M), **bad))


# ---------------------------------------------------------------------------------------------------------------- GPU

# Every edge of the kernels' tiling: the column pass's strip of 64 rows and 256 columns, the row pass's tile of 8 rows x 256 columns, the
# fused kernel's 64 x 64 cells - and maps smaller than any halo.
FIELD_SHAPES = [(1, 1), (1, 70), (70, 1), (63, 64), (65, 257), (160, 160), (9, 513)]
# R below and above every map; 32 | 33 is where the fused kernel (sv_debug_clearance's variant 1) gives way to the two kernels - the only
# place the radius changes the path taken; 63 | 64 | 65 walk the column pass's halo to just short of, onto and past a whole strip.
FIELD_RADII = (1, 2, 31, 32, 33, 63, 64, 65, 254)
VARIANTS = (0, 1, 2, 3)


def _field_cases(rng, rows, cols):
    """name -> (logodds, last_seen or None, t_occ, unknown)."""
    base = np.full((rows, cols), -5, np.int16)
    corners, border = base.copy(), base.copy()
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = 7
    border[[0, -1], :] = 7
    border[:, [0, -1]] = 7
    sparse = base.copy()
    sparse[rng.random((rows, cols)) < 0.001] = 7
    sparse[rng.integers(rows), rng.integers(cols)] = 7
    wide = rng.integers(-32768, 32768, (rows, cols)).astype(np.int16)  # 30 % at or above 13107
    top = np.full((rows, cols), 32766, np.int16)
    top[rng.integers(rows), rng.integers(cols)] = 32767
    seen = rng.choice(np.array([-1, 0, 5], np.int32), (rows, cols), p=[0.01, 0.495, 0.495])
    return {"none": (base, None, 0, 0), "all": (base + 10, None, 0, 0), "corners": (corners, None, 7, 0), "border": (border, seen, 7, 0), "sparse": (sparse, None, 0, 0),
            "dense": (wide, None, 13107, 0), "everything": (wide, seen, -32768, 0), "top": (top, None, 32767, 0), "unknown": (sparse, seen, 0, 1),
            "unknown_off": (sparse, seen, 0, 0), "unknown_only": (base, seen, 32767, 1)}


def _field_gpu(eng, case, R, variant=0, counter=None):
    L, S, t_occ, unknown = case
    try:
        assert eng.debug_clearance(variant, counter) == 0
        return eng.occupancy_clearance(_cuda(L), R, t_occ, None if S is None else _cuda(S), unknown).cpu().numpy()
    finally:
        eng.debug_clearance(0, None)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", FIELD_SHAPES, ids=lambda s: "%dx%d" % s)
def test_field_equals_the_definition(sv, eng, shape):
    rows, cols = shape
    rng = np.random.default_rng(1000 * rows + cols)
    cases = _field_cases(rng, rows, cols)
    for name, case in cases.items():
        for R in FIELD_RADII:
            want = sv.occupancy_clearance(case[0], R, case[2], case[1], bool(case[3]))
            for variant in VARIANTS:
                got = _field_gpu(eng, case, R, variant)
                assert _bits(got, want), (shape, name, R, variant, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
    assert (sv.occupancy_clearance(cases["none"][0], 254, 0) == F).all() and not sv.occupancy_clearance(cases["all"][0], 1, 0).any()
    if rows > 2 and cols > 2:  # sources on the border only: the middle is as far from them as from the map's edge, and not nearer
        want = sv.occupancy_clearance(cases["border"][0], 254, 7)
        assert want[rows // 2, cols // 2] == min(rows // 2, (rows - 1) - rows // 2, cols // 2, (cols - 1) - cols // 2) ** 2


@pytest.mark.gpu
def test_field_mechanics(sv, eng):
    """The tap counter with and without the early exit, garbage in the output and the workspace, a stream of its own, repeats, and the C
    entry's refusals on device buffers, which stay as they were."""
    import torch
    rows, cols, R = 65, 257, 33
    rng = np.random.default_rng(5)
    case = _field_cases(rng, rows, cols)["dense"]
    want = sv.occupancy_clearance(case[0], R, case[2])
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    taps = {}
    for variant, radius in ((3, R), (2, R), (0, R), (3, 32), (1, 32)):
        counter.zero_()
        torch.cuda.synchronize()
        got = _field_gpu(eng, case, radius, variant, counter)
        torch.cuda.synchronize()
        taps[variant, radius] = int(counter.item())
        assert _bits(got, want if radius == R else sv.occupancy_clearance(case[0], radius, case[2]))
    print("taps", taps)
    assert taps[3, R] == rows * cols * (2 * R + 1) and taps[3, 32] == rows * cols * 65
    assert 0 < taps[2, R] < taps[3, R] // 4 and taps[0, R] == taps[2, R] and 0 < taps[1, 32] < taps[3, 32] // 4
    Lib = eng.clearance_lib()
    L, S = _cuda(case[0]), _cuda(rng.choice(np.array([-1, 0, 5], np.int32), (rows, cols)))
    want_unknown = sv.occupancy_clearance(case[0], R, case[2], S.cpu().numpy(), True)
    need = ctypes.c_size_t()
    assert Lib.sv_clearance_workspace(rows, cols, ctypes.byref(need)) == 0

    def raw(t_d2, t_ws, stream=None, **kw):
        a = dict(dict(logodds=L.data_ptr(), last_seen=S.data_ptr(), rows=rows, cols=cols, radius=R, t_occ=case[2], unknown=1, d2=t_d2.data_ptr(), ws=t_ws.data_ptr(),
                      ws_bytes=t_ws.numel(), stream=(torch.cuda.current_stream() if stream is None else stream).cuda_stream), **kw)
        return _c_field_call(Lib, a)

    side = torch.cuda.Stream()
    seen = set()
    for rep, stream in enumerate((None, None, side, side, None)):
        d2 = _cuda(np.full((rows, cols), 0x5A5A, np.uint16))
        ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        assert raw(d2, ws, stream) == 0
        if stream is not None:
            torch.cuda.current_stream().wait_stream(stream)
        assert _bits(d2.cpu().numpy(), want_unknown), rep
        seen.add(d2.cpu().numpy().tobytes())
    assert len(seen) == 1
    # into the caller's tensors through the engine
    out, ws = _cuda(np.full((rows, cols), 0x5A5A, np.uint16)), torch.full((need.value + 5,), 0xA5, dtype=torch.uint8, device="cuda")
    assert eng.occupancy_clearance(L, R, case[2], out=out, workspace=ws) is out and _bits(out.cpu().numpy(), want)
    # refused on the device as on the host: nothing is written
    d2 = _cuda(np.full((rows, cols), 0x5A5A, np.uint16))
    ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda")
    for kw in _BAD_FIELD + [dict(ws_bytes=need.value - 16), dict(last_seen=None), dict(logodds=None), dict(d2=L.data_ptr()), dict(d2=ws.data_ptr()), dict(ws=ws.data_ptr() + 8)]:
        assert raw(d2, ws, **kw) == SV_ERR_ARG and Lib.sv_last_error(None).startswith(b"sv_clearance:"), sorted(kw)
    torch.cuda.synchronize()
    assert (d2.cpu().numpy() == 0x5A5A).all() and (ws == 0xA5).all() and _bits(L.cpu().numpy(), case[0])
    for bad in (dict(logodds=L.int()), dict(logodds=L.cpu()), dict(logodds=L.t()), dict(radius=255), dict(t_occ=40000), dict(unknown=True), dict(last_seen=S.long()),
                dict(last_seen=S[:3]), dict(out=out.view(torch.int16)), dict(out=out[:3]), dict(workspace=ws[:100]), dict(unknown=3, last_seen=S)):
        with pytest.raises(ValueError):
            eng.occupancy_clearance(**dict(dict(logodds=L, radius=R, t_occ=0), **bad))


PATH_COUNTS = (1, 63, 64, 65, 300)   # a workgroup checks four paths, a wavefront each
PATH_STEPS = (1, 63, 64, 65, 200)    # with the discs: every number of lookups around a wavefront's 64 lanes, and many rounds of them


def _paths_gpu(eng, d2, words, poses, centres, r2, radius):
    res = eng.clearance_paths(d2, words, poses, (centres, r2), radius)
    return {k: getattr(res, k).cpu().numpy() for k in PATH_KEYS}


@pytest.mark.gpu
@pytest.mark.parametrize("n_discs", [1, 3, 64])
@pytest.mark.parametrize("map_name", sorted(SMALL_MAPS))
def test_paths_equal_the_definition(sv, eng, map_name, n_discs):
    """Paths inside the map, clipped at each of its edges, missing it, and with words that are not finite; a field with every kind of value;
    squared radii of 0 and of R^2."""
    words = _small_words(sv, map_name)
    rng = np.random.default_rng(300 + n_discs)
    R = 9
    d2 = rng.choice(np.array([0, 1, 2, 50, 81, F], np.uint16), (160, 160), p=[0.02, 0.02, 0.02, 0.04, 0.1, 0.8])
    t_d2 = _cuda(d2)
    centres = np.round(rng.uniform(-3.0, 3.0, (n_discs, 2)) * 8) / 8
    r2 = rng.choice(np.array([0, 1, 49, 80, 81], np.int32), n_discs)
    r2[0], r2[-1] = (0, 81) if n_discs > 1 else (81, 81)
    hits = clipped = 0
    for K in PATH_COUNTS:
        for T in PATH_STEPS:
            poses = _poses_around(sv, rng, words, K * T).reshape(K, T, 4)
            want = sv.clearance_paths(d2, words, poses, centres, r2, R)
            got = _paths_gpu(eng, t_d2, words, poses, centres, r2, R)
            assert all(_bits(got[k], want[k]) for k in PATH_KEYS), (map_name, n_discs, K, T, [k for k in PATH_KEYS if not _bits(got[k], want[k])])
            hits += int(((want["first_hit"] > 0) & (want["first_hit"] < T)).sum())
            clipped += int(((want["n_outside"] > 0) & (want["n_outside"] < T * n_discs)).sum())
    assert hits > 0 and clipped > 0
    # a path whose only hit is its last step, one that stands on an obstacle from step 0, one that is clear: the field is far everywhere
    # but at the first disc's cell under one pose
    T = 65
    poses = _poses_around(sv, rng, words, 3 * T)[:T]  # the inside ones
    ok, r, c = sv.clearance_cells(words, poses, centres)
    assert ok.all()
    paths = np.stack([poses, poses[::-1], poses])
    far = np.full((160, 160), F, np.uint16)
    far[r[T - 1, -1], c[T - 1, -1]] = r2[-1]  # the boundary d2 == r2
    want = sv.clearance_paths(far, words, paths, centres, r2, R)
    first = want["first_hit"].tolist()
    assert first == [T - 1, 0, T - 1] and want["n_outside"].tolist() == [0, 0, 0]
    got = _paths_gpu(eng, _cuda(far), words, paths, centres, r2, R)
    assert all(_bits(got[k], want[k]) for k in PATH_KEYS)
    none = sv.clearance_paths(np.full((160, 160), F, np.uint16), words, paths, centres, r2, R)
    assert none["first_hit"].tolist() == [T] * 3 and _bits(_paths_gpu(eng, _cuda(np.full((160, 160), F, np.uint16)), words, paths, centres, r2, R)["first_hit"], none["first_hit"])


@pytest.mark.gpu
def test_paths_buffers_streams_and_refusals(sv, eng):
    import torch
    words = _small_words(sv, "plain")
    rng = np.random.default_rng(77)
    d2 = rng.choice(np.array([0, 3, 16, F], np.uint16), (160, 160), p=[0.05, 0.05, 0.1, 0.8])
    poses = _poses_around(sv, rng, words, 70 * 9).reshape(70, 9, 4)
    centres, r2 = sv.clearance_discs(FOOTPRINT_M, 4)
    want = sv.clearance_paths(d2, words, poses, centres, r2, 4)
    Lib, spec = eng.clearance_lib(), eng._occupancy_map_struct(words)
    t_d2, t_poses = _cuda(d2), _cuda(poses)

    def raw(outs, stream=None, **kw):
        a = dict(dict(d2=t_d2.data_ptr(), map=spec, poses=t_poses.data_ptr(), n_paths=70, n_steps=9, centres=centres.ctypes.data, r2=r2.ctypes.data, n_discs=3, radius=4,
                      first_hit=outs[0].data_ptr(), min_d2=outs[1].data_ptr(), n_outside=outs[2].data_ptr(),
                      stream=(torch.cuda.current_stream() if stream is None else stream).cuda_stream), **kw)
        return _c_paths_call(Lib, a)

    side = torch.cuda.Stream()
    for stream in (None, side, None):
        outs = [torch.full((70,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(3)]
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        assert raw(outs, stream) == 0
        if stream is not None:
            torch.cuda.current_stream().wait_stream(stream)
        assert all(_bits(o.cpu().numpy(), want[k]) for o, k in zip(outs, PATH_KEYS))
    outs = [torch.full((70,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(3)]
    big = np.array([4, 17, 4], np.int32)
    for kw in _BAD_PATHS + [dict(r2=big.ctypes.data), dict(radius=1), dict(map=None), dict(d2=None), dict(poses=t_poses.data_ptr() + 4), dict(min_d2=None)]:
        assert raw(outs, **kw) == SV_ERR_ARG and Lib.sv_last_error(None).startswith(b"sv_clearance_paths"), sorted(kw)
    assert raw(outs, n_paths=0) == 0
    torch.cuda.synchronize()
    assert all((o == 0x5A5A5A5A).all() for o in outs)
    for bad in (dict(d2=t_d2.view(torch.int16)), dict(d2=t_d2.cpu()), dict(d2=t_d2[:100]), dict(poses=t_poses.float()), dict(poses=poses[0]), dict(discs=(centres, big)), dict(radius=255),
                dict(map=dict(words, rows=0))):
        with pytest.raises(ValueError):
            eng.clearance_paths(**dict(dict(d2=t_d2, map=words, poses=t_poses, discs=(centres, r2), radius=4), **bad))
    assert eng.clearance_paths(t_d2, words, np.zeros((0, 5, 4)), (centres, r2), 4).first_hit.shape == (0,)


@pytest.mark.gpu
def test_map_class_on_the_device(sv, eng):
    """rig.OccupancyMap on the device against the class on CPU tensors: the recovery scene fused, its field, a fan of paths, and the field
    again after another frame."""
    world, cpu = _fused_recovery_maps(sv, ["cuda", "cpu"])
    d2, d2_cpu = world.clearance(1.0), cpu.clearance(1.0)
    assert d2.is_cuda and world.clearance_radius == cpu.clearance_radius == 4 and _bits(d2.cpu().numpy(), d2_cpu.numpy()) and (d2_cpu.numpy() == 0).any()
    fan = _fan(sv)
    res, res_cpu = world.check_paths(fan, FOOTPRINT_M), cpu.check_paths(fan, FOOTPRINT_M)
    assert all(_bits(getattr(res, k).cpu().numpy(), getattr(res_cpu, k).numpy()) for k in PATH_KEYS) and (res_cpu.first_hit < 20).any()
    before = d2_cpu.numpy().copy()
    for m in (world, cpu):
        m.update(_recovery_state()[None], sv.occupancy_pose(9.0, 4.0, -0.8)[None], RECOVERY_FRAME)
    again, again_cpu = world.clearance(1.0), cpu.clearance(1.0)
    assert again is d2 and _bits(again.cpu().numpy(), again_cpu.numpy()) and not np.array_equal(again_cpu.numpy(), before)
    assert _bits(world.clearance(2.0, occupied=0, unknown=True).cpu().numpy(), cpu.clearance(2.0, occupied=0, unknown=True).numpy()) and world.clearance_radius == 8
    res, res_cpu = world.check_paths(_cuda(fan), FOOTPRINT_M), cpu.check_paths(fan, FOOTPRINT_M)
    assert all(_bits(getattr(res, k).cpu().numpy(), getattr(res_cpu, k).numpy()) for k in PATH_KEYS)


@pytest.mark.gpu
def test_cli_writes_the_clearance_field(sv, eng, drive, tmp_path):
    from PIL import Image
    _, states, _, _, _ = drive
    n = 2
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    ls, rs = _drive_frames(n)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    xyyaw = np.array([[0.0, 0.0, 0.0], [0.9, 0.1, 0.02]])
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("".join("%r %r %r\n" % tuple(float(v) for v in row) for row in xyyaw))
    out = str(tmp_path / "map.png")
    common = ["-k", str(tmp_path / "kitti"), "--batch", "2"]
    for bad in (["--clearance", "2.0"], ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--clearance", "25.5"],
                ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--clearance", "-1"]):
        with pytest.raises(SystemExit):
            sv.main(common + bad)
    assert not os.path.exists(out)
    sv.main(common + ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--clearance", "2.0"])
    ranges = sv.occupancy_map_cover(xyyaw, sv.CLI_TOP_VIEW["x_range"], sv.CLI_TOP_VIEW["y_range"])
    cpu = util.pkg("rig").OccupancyMap(ranges[0], ranges[1], 10, device="cpu")
    cpu.update(states[:2], sv.occupancy_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2]), CLI_GRID)
    assert np.array_equal(np.asarray(Image.open(out)), sv.OCCUPANCY_PNG[cpu.state().numpy()])
    got = np.asarray(Image.open(str(tmp_path / "map.clearance.png")))
    want = sv.clearance_png(cpu.clearance(2.0).numpy())
    assert got.dtype == np.uint8 and np.array_equal(got, want) and want.min() == 0 and (want == 255).any() and want[want < 255].max() <= 20
