"""The world-fixed occupancy map (include/stereo_vision_hip.h (K)): the numpy definition in stereo_vision.sv on hand-built cases, the order
under the clamp, the scroll, recenter, the argument checks in Python and in the C ABI, and the HIP kernel - C entry, engine, rig.OccupancyMap
and the CLI - against the definition.

Everything is compared exactly.  That is derived, not chosen: the centre of a map cell, its place in a frame and the range tests are
products, sums and comparisons of doubles in a stated order - -ffp-contract=off on the device, and numpy never fuses - and everything behind
trunc() is integer work in a fixed order per cell."""
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
IDENTITY, QUARTER = (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _same(got, want):
    return _bits(got["logodds"], want["logodds"]) and _bits(got["last_seen"], want["last_seen"])


# ---------------------------------------------------------------------------------------------------------------- CPU

# A frame grid of 9 x 5 cells: x 0..8, y -2..2 at scale 1, so FR1 = 8, FC1 = 2 and a point (Xf, Yf) lies in cell (8 - trunc(Xf), 2 - trunc(Yf)).
HAND_FRAME = dict(x_range=(0, 8), y_range=(-2, 2), scale=1)
HAND_STATE = np.array([[0, 1, 2, 1, 0],
                       [1, 2, 1, 0, 2],
                       [2, 2, 0, 1, 1],
                       [0, 1, 1, 2, 2],
                       [1, 0, 2, 2, 1],
                       [2, 1, 0, 0, 1],
                       [1, 1, 2, 1, 0],
                       [0, 2, 1, 2, 1],
                       [2, 0, 1, 1, 2]], np.uint8)
O, F = 85, -40  # one occupied, one free observation with the default words
# The identity pose into the 8 x 4 map with top 8, left 2: the centres are Xw = 7.5 - r and Yw = 1.5, 0.5, -0.5, -1.5, all strictly inside
# the frame.  Frame row 8 - trunc(7.5 - r) = r + 1; frame column 2 - trunc(Yw) = 1, 2, 2, 3: both centres next to 0 fall into the frame's
# double-width column.  So map row r is HAND_STATE[r + 1][[1, 2, 2, 3]].
HAND_IDENTITY = np.array([[O, F, F, 0],
                          [O, 0, 0, F],
                          [F, F, F, O],
                          [0, O, O, O],
                          [F, 0, 0, 0],
                          [F, O, O, F],
                          [O, F, F, O],
                          [0, F, F, F]], np.int16)
# The exact quarter turn (c, s) = (0, 1) into the 8 x 9 map with top 4, left 9: Xf = Yw = 8.5 - c, inside 0..8 for c = 1 .. 8, frame row
# 8 - trunc(8.5 - c) = c; Yf = -Xw = r - 3.5, inside -2..2 for r = 2 .. 5, frame column 2 - trunc(r - 3.5) = 3, 2, 2, 1.  So map (r, c) is
# HAND_STATE[c][3, 2, 2, 1 for r = 2 .. 5]: the frame's columns 3, 2, 2, 1 read downwards, laid out along the map's rows.
HAND_QUARTER = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0],
                         [0, 0, 0, 0, 0, 0, 0, 0, 0],
                         [0, 0, F, O, O, 0, F, O, F],
                         [0, F, 0, F, O, 0, O, F, F],
                         [0, F, 0, F, O, 0, O, F, F],
                         [0, O, O, F, 0, F, F, O, 0],
                         [0, 0, 0, 0, 0, 0, 0, 0, 0],
                         [0, 0, 0, 0, 0, 0, 0, 0, 0]], np.int16)


def test_hand_built_cases(sv):
    m = sv.occupancy_map_params((0, 8), (-2, 2), 1)
    assert m == dict(top=8, left=2, rows=8, cols=4, scale=1, l_occ=85, l_free=40, l_min=-200, l_max=350)
    Xw, Yw = sv.occupancy_map_centres(m)
    assert Xw.tolist() == [7.5 - r for r in range(8)] and Yw.tolist() == [1.5, 0.5, -0.5, -1.5]
    got = sv.occupancy_fuse(HAND_STATE, [IDENTITY], HAND_FRAME, m)
    assert got["logodds"].dtype == np.int16 and got["last_seen"].dtype == np.int32
    assert np.array_equal(got["logodds"], HAND_IDENTITY) and np.array_equal(got["last_seen"], np.where(HAND_IDENTITY != 0, 0, -1))
    q = sv.occupancy_map_params((-4, 4), (0, 9), 1)
    assert (q["top"], q["left"], q["rows"], q["cols"]) == (4, 9, 8, 9)
    got = sv.occupancy_fuse(HAND_STATE[None], np.array([QUARTER]), HAND_FRAME, q, seq0=7)
    assert np.array_equal(got["logodds"], HAND_QUARTER) and np.array_equal(got["last_seen"], np.where(HAND_QUARTER != 0, 7, -1))
    assert HAND_QUARTER[2:6].any(axis=1).all() and not HAND_QUARTER[[0, 1, 6, 7]].any()
    # occupancy_pose: numpy's cos and sin, (x, y) as they are
    p = sv.occupancy_pose([1.5, -2.0], [0.25, 3.0], [0.0, 0.5])
    assert p.dtype == np.float64 and p.shape == (2, 4) and p[0].tolist() == [1.5, 0.25, 1.0, 0.0] and p[1].tolist() == [-2.0, 3.0, np.cos(0.5), np.sin(0.5)]
    assert sv.occupancy_pose(1.0, 2.0, 0.0).shape == (4,)
    # a translation by whole cells moves the picture by whole cells: the vehicle one cell ahead and one to the left
    moved = sv.occupancy_fuse(HAND_STATE, [(1.0, 1.0, 1.0, 0.0)], HAND_FRAME, dict(m, top=9, left=3))
    assert np.array_equal(moved["logodds"], HAND_IDENTITY)


def test_order_under_the_clamp(sv):
    m = sv.occupancy_map_params((0, 8), (-2, 2), 1)
    occ, free = np.full((9, 5), 2, np.uint8), np.full((9, 5), 1, np.uint8)
    poses = [IDENTITY] * 6
    a = sv.occupancy_fuse(np.stack([occ] * 5 + [free]), poses, HAND_FRAME, m)
    b = sv.occupancy_fuse(np.stack([free] + [occ] * 5), poses, HAND_FRAME, m)
    assert (a["logodds"] == 310).all() and (b["logodds"] == 350).all()  # 4 x 85 = 340, 425 -> 350, - 40; and -40 + 5 x 85 = 385 -> 350
    assert (a["last_seen"] == 5).all() and (b["last_seen"] == 5).all()
    # l_min is reached and held: -40 x 5 = -200, and stays
    c = sv.occupancy_fuse(np.stack([free] * 9), [IDENTITY] * 9, HAND_FRAME, m)
    assert (c["logodds"] == -200).all()
    d = sv.occupancy_fuse(np.stack([free] * 4), [IDENTITY] * 4, HAND_FRAME, dict(m, l_min=-100, l_free=70))
    assert (d["logodds"] == -100).all()
    # a state byte above 2 is ignored, as 0 is: neither logodds nor last_seen move
    odd = np.stack([np.full((9, 5), 3, np.uint8), np.full((9, 5), 255, np.uint8), np.zeros((9, 5), np.uint8)])
    e = sv.occupancy_fuse(odd, [IDENTITY] * 3, HAND_FRAME, m, logodds=a["logodds"], last_seen=a["last_seen"], seq0=50)
    assert _same(e, a)
    # a pose with a word that is not finite skips its frame
    for k in range(4):
        for bad in (NAN, INF, -INF):
            pose = list(IDENTITY)
            pose[k] = bad
            f = sv.occupancy_fuse(np.stack([occ, free]), [pose, IDENTITY], HAND_FRAME, m)
            assert (f["logodds"] == -40).all() and (f["last_seen"] == 1).all(), (k, bad)
    # last_seen takes seq0 + b, over two chained calls
    first = sv.occupancy_fuse(np.stack([HAND_STATE, np.zeros((9, 5), np.uint8)]), [IDENTITY] * 2, HAND_FRAME, m, seq0=10)
    assert np.array_equal(first["last_seen"], np.where(HAND_IDENTITY != 0, 10, -1))
    only_left = np.zeros((9, 5), np.uint8)
    only_left[:, 1] = 2
    second = sv.occupancy_fuse(np.stack([np.zeros((9, 5), np.uint8), only_left]), [IDENTITY] * 2, HAND_FRAME, m, first["logodds"], first["last_seen"], seq0=12)
    want = np.where(HAND_IDENTITY != 0, 10, -1)
    want[:, 0] = 13
    assert np.array_equal(second["last_seen"], want) and np.array_equal(second["logodds"][:, 1:], HAND_IDENTITY[:, 1:])
    assert np.array_equal(second["logodds"][:, 0], HAND_IDENTITY[:, 0] + 85)
    # no last_seen kept
    assert sv.occupancy_fuse(HAND_STATE, [IDENTITY], HAND_FRAME, m, last_seen=False)["last_seen"] is None


SHIFTS = [(0, 0), (3, -2), (-8, 0), (0, 4), (100, 3), (-3, -100000), (2 ** 31 - 1, 0), (1, 1 - 2 ** 31)]


def _plain_scroll(a, shift, fill):
    """The scroll, cell by cell."""
    out = np.full_like(a, fill)
    for r in range(a.shape[0]):
        for c in range(a.shape[1]):
            ri, ci = r + shift[0], c + shift[1]
            if 0 <= ri < a.shape[0] and 0 <= ci < a.shape[1]:
                out[r, c] = a[ri, ci]
    return out


def test_scroll(sv):
    rng = np.random.default_rng(5)
    m = sv.occupancy_map_params((0, 8), (-2, 2), 1)
    L0 = rng.integers(-200, 351, (8, 4)).astype(np.int16)
    S0 = rng.integers(-1, 40, (8, 4)).astype(np.int32)
    none = np.zeros((0, 9, 5), np.uint8), np.zeros((0, 4))
    for shift in SHIFTS:
        got = sv.occupancy_fuse(none[0], none[1], HAND_FRAME, m, L0, S0, shift=shift)  # without a frame the map's place plays no part
        assert np.array_equal(got["logodds"], _plain_scroll(L0, shift, 0)) and np.array_equal(got["last_seen"], _plain_scroll(S0, shift, -1)), shift
    assert not sv.occupancy_fuse(none[0], none[1], HAND_FRAME, m, L0, S0, shift=(-8, 0))["logodds"].any()
    # two scrolls by part of the shift equal one by the whole shift - as long as nothing that comes back had left the map in between
    for whole, part in (((3, -2), (1, -1)), ((-5, 3), (-2, 0)), ((8, 0), (4, 0)), ((2, 2), (5, 5))):
        rest = (whole[0] - part[0], whole[1] - part[1])
        one = sv.occupancy_fuse(none[0], none[1], HAND_FRAME, m, L0, S0, shift=whole)
        half = sv.occupancy_fuse(none[0], none[1], HAND_FRAME, m, L0, S0, shift=part)
        two = sv.occupancy_fuse(none[0], none[1], HAND_FRAME, m, half["logodds"], half["last_seen"], shift=rest)
        same_way = part[0] * rest[0] >= 0 and part[1] * rest[1] >= 0
        assert _same(one, two) == same_way, (whole, part)
    # a scroll followed by an update equals the update done directly on a map with top and left moved
    for shift in ((3, -2), (-1, 1), (0, 0)):
        moved = dict(m, top=m["top"] - shift[0], left=m["left"] - shift[1])
        poses = sv.occupancy_pose([0.5, -2.0], [0.25, 1.0], [0.0, 0.3])
        states = np.stack([HAND_STATE, HAND_STATE[::-1]])
        fused = sv.occupancy_fuse(states, poses, HAND_FRAME, moved, L0, S0, seq0=40, shift=shift)
        scrolled = sv.occupancy_fuse(none[0], none[1], HAND_FRAME, moved, L0, S0, shift=shift)
        direct = sv.occupancy_fuse(states, poses, HAND_FRAME, moved, scrolled["logodds"], scrolled["last_seen"], seq0=40)
        by_hand = sv.occupancy_fuse(states, poses, HAND_FRAME, moved, _plain_scroll(L0, shift, 0), _plain_scroll(S0, shift, -1), seq0=40)
        assert _same(fused, direct) and _same(fused, by_hand) and (fused["last_seen"] >= 40).any(), shift


def test_recenter_and_the_map_class_on_cpu_tensors(sv):
    """rig.OccupancyMap on CPU tensors runs the numpy definition: the host logic - recenter, state, the sequence numbers - without a GPU."""
    import torch
    rigmod = util.pkg("rig")
    for x, y in ((0.0, 0.0), (3.3, -7.2), (-3.3, 7.2), (-120.04, -0.05), (1000.0, 999.95), (-0.0499, 0.0501)):
        for rng_x, rng_y, scale in (((0, 8), (-2, 2), 1), ((-3, 4), (-2, 3), 10), ((0, 5), (0, 3), 3)):
            m = rigmod.OccupancyMap(rng_x, rng_y, scale, device="cpu")
            before = dict(m.words)
            shift = m.recenter(x, y)
            assert (m.words["top"], m.words["left"]) == (before["top"] - shift[0], before["left"] - shift[1])
            Xw, Yw = m.centres()
            r, c = m.words["rows"] // 2, m.words["cols"] // 2
            half = 0.5 / scale
            # half a cell, and the rounding of the centre's one product and of half itself: a few ulp of the coordinate
            assert abs(Xw[r] - x) <= half + 2.0 ** -50 * (abs(x) + 1) and abs(Yw[c] - y) <= half + 2.0 ** -50 * (abs(y) + 1), (x, y, scale)
            assert m.recenter(x, y) == (0, 0)
    with pytest.raises(ValueError):
        rigmod.OccupancyMap((0, 8), (-2, 2), 1, device="cpu").recenter(NAN, 0)
    with pytest.raises(ValueError):
        rigmod.OccupancyMap((0, 8), (-2, 2), 1, device="cpu").recenter(2.0 ** 24, 0)
    # update, recenter, update: the same as the definition with the scroll in between
    m = rigmod.OccupancyMap((0, 8), (-2, 2), 1, device="cpu")
    states = np.stack([HAND_STATE, HAND_STATE[::-1], HAND_STATE[:, ::-1]])
    poses = sv.occupancy_pose([0.0, 1.0, 2.5], [0.0, 0.5, 1.0], [0.0, 0.1, 0.2])
    m.update(torch.from_numpy(states[:2]), poses[:2], HAND_FRAME)
    assert m.seq == 2
    words0 = dict(m.words)
    a = sv.occupancy_fuse(states[:2], poses[:2], HAND_FRAME, words0)
    assert np.array_equal(m.logodds.numpy(), a["logodds"]) and np.array_equal(m.last_seen.numpy(), a["last_seen"])
    shift = m.recenter(2.5, 1.0)
    assert shift != (0, 0)
    m.update(torch.from_numpy(states[2:]), torch.from_numpy(poses[2:]), HAND_FRAME)
    b = sv.occupancy_fuse(states[2:], poses[2:], HAND_FRAME, m.words, a["logodds"], a["last_seen"], seq0=2, shift=shift)
    assert m.seq == 3 and np.array_equal(m.logodds.numpy(), b["logodds"]) and np.array_equal(m.last_seen.numpy(), b["last_seen"]) and (b["last_seen"] == 2).any()
    # state: thresholds on logodds where the cell was ever seen
    for kw in (dict(), dict(occupied=100, free=-50), dict(occupied=0, free=0)):
        want = sv.occupancy_map_state(b["logodds"], b["last_seen"], kw.get("occupied", 85), kw.get("free", -40))
        plain = np.zeros_like(want)
        plain[(b["last_seen"] >= 0) & (b["logodds"] <= kw.get("free", -40))] = 1
        plain[(b["last_seen"] >= 0) & (b["logodds"] >= kw.get("occupied", 85))] = 2
        got = m.state(**kw)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want) and np.array_equal(want, plain)
    assert len(np.unique(m.state().numpy())) == 3
    m.reset()
    assert m.seq == 0 and not m.logodds.any() and (m.last_seen == -1).all() and m.words["top"] == words0["top"] - shift[0]
    with pytest.raises(ValueError):
        m.update(torch.from_numpy(states), poses)  # no frame grid
    with pytest.raises(ValueError):
        m.update(torch.from_numpy(states), poses[:2], HAND_FRAME)


_BAD_MAPS = [dict(rows=0), dict(cols=0), dict(rows=32769), dict(cols=40000), dict(rows=-3), dict(scale=0), dict(scale=-1), dict(top=2 ** 24), dict(top=-2 ** 24),
             dict(left=2 ** 24), dict(left=-2 ** 24 - 5), dict(l_occ=0), dict(l_occ=32768), dict(l_free=0), dict(l_free=-4), dict(l_free=40000),
             dict(l_min=-32768), dict(l_min=1), dict(l_max=-1), dict(l_max=32768), dict(l_min=0, l_max=0)]
_GOOD_MAP = dict(top=8, left=2, rows=8, cols=4, scale=1, l_occ=85, l_free=40, l_min=-200, l_max=350)
_BAD_FRAMES = [dict(x_range=(0.5, 4)), dict(x_range=(4, 4)), dict(y_range=(2, -2)), dict(scale=0), dict(x_range=(0, 40000))]


def _c_map(eng, reserved=None, **kw):
    sp = eng.SvOccupancyMapSpec()
    for k, v in dict(_GOOD_MAP, **kw).items():
        setattr(sp, k, v)
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


def test_validation_needs_no_device(sv, eng):
    """Every refused argument raises ValueError in Python; the C entry returns SV_ERR_ARG on host buffers, which stay untouched: the checks
    run before any HIP call."""
    one = (HAND_STATE[None], [IDENTITY], HAND_FRAME)
    for bad in _BAD_MAPS + [dict(rows=1.5), dict(l_occ=True)]:
        with pytest.raises(ValueError):
            sv.occupancy_fuse(*one, dict(_GOOD_MAP, **bad))
        with pytest.raises(ValueError):
            sv.occupancy_map_words(dict(_GOOD_MAP, **bad))
    for bad in (dict(x_range=(0.5, 8)), dict(x_range=(8, 8)), dict(y_range=(2, -2)), dict(scale=0), dict(scale=1.5), dict(x_range=(0, 40000)), dict(scale=2 ** 22),
                dict(l_occ=0), dict(l_min=5), dict(l_min=0, l_max=0)):
        with pytest.raises(ValueError):
            sv.occupancy_map_params(**dict(dict(x_range=(0, 8), y_range=(-2, 2), scale=1), **bad))
        with pytest.raises(ValueError):
            eng.occupancy_map_spec(**dict(dict(x_range=(0, 8), y_range=(-2, 2), scale=1), **bad))
    for bad in _BAD_FRAMES:
        with pytest.raises(ValueError):
            sv.occupancy_fuse(HAND_STATE[None], [IDENTITY], dict(HAND_FRAME, **bad), _GOOD_MAP)
    for bad in (dict(state=HAND_STATE[None, :8]), dict(state=HAND_STATE[None].astype(np.int32)), dict(poses=[IDENTITY] * 2), dict(poses=[IDENTITY[:3]]), dict(seq0=-1),
                dict(seq0=2 ** 31 - 1), dict(seq0=0.5), dict(shift=(1,)), dict(shift=(0.5, 0)), dict(logodds=np.zeros((8, 4), np.int32)),
                dict(logodds=np.zeros((4, 8), np.int16)), dict(last_seen=np.zeros((8, 4), np.int16))):
        a = dict(dict(state=HAND_STATE[None], poses=[IDENTITY], frame_grid=HAND_FRAME, map=_GOOD_MAP), **bad)
        with pytest.raises(ValueError):
            sv.occupancy_fuse(**a)
    sp = eng.occupancy_map_spec((-10, 60), (-30, 30), 10, l_occ=90)
    assert [sp.top, sp.left, sp.rows, sp.cols, sp.scale, sp.l_occ, sp.l_free, sp.l_min, sp.l_max] == [600, 300, 700, 600, 10, 90, 40, -200, 350]
    assert list(sp.reserved) == [0] * 7 and ctypes.sizeof(sp) == 64

    L = eng.occupancy_map_lib()
    frame, _, _ = eng.occupancy_spec((0, 8), (-2, 2), (-1, 1), 1)
    bufs = {k: np.full(4096, 0x5A, np.uint8) for k in ("state", "poses", "l_in", "s_in", "l_out", "s_out")}
    ptr = lambda name: bufs[name].ctypes.data  # noqa: E731
    assert all(ptr(k) % 8 == 0 for k in bufs)
    base = dict(state=ptr("state"), poses=ptr("poses"), batch=2, seq0=0, frame=frame, map=_c_map(eng), shift=(0, 0), l_in=ptr("l_in"), s_in=ptr("s_in"), l_out=ptr("l_out"),
                s_out=ptr("s_out"))

    def call(**kw):
        a = dict(base, **kw)
        return L.sv_occupancy_fuse_device(a["state"], a["poses"], a["batch"], a["seq0"], None if a["frame"] is None else ctypes.byref(a["frame"]),
                                          None if a["map"] is None else ctypes.byref(a["map"]), a["shift"][0], a["shift"][1], a["l_in"], a["s_in"], a["l_out"], a["s_out"], None)

    bad_frames = []
    for kw in _BAD_FRAMES:
        f, _, _ = eng.occupancy_spec((0, 8), (-2, 2), (-1, 1), 1)
        for k, v in kw.items():
            if k == "scale":
                f.scale = v
            else:
                getattr(f, k)[:] = [float(t) for t in v]
        bad_frames.append(f)
    f, _, _ = eng.occupancy_spec((0, 8), (-2, 2), (-1, 1), 1)
    f.reserved[2] = 1
    bad_frames.append(f)
    cases = [dict(frame=None), dict(map=None), dict(state=None), dict(poses=None), dict(l_in=None), dict(l_out=None), dict(s_in=None), dict(s_out=None),
             dict(poses=ptr("poses") + 4), dict(l_in=ptr("l_in") + 1), dict(l_out=ptr("l_out") + 1), dict(s_in=ptr("s_in") + 2), dict(s_out=ptr("s_out") + 1),
             dict(batch=-1), dict(batch=65536), dict(seq0=-1), dict(seq0=2 ** 31 - 2), dict(seq0=2 ** 31 - 1, batch=1),
             dict(l_out=ptr("l_in"), shift=(1, 0)), dict(l_out=ptr("l_in") + 2 * 31, s_out=ptr("s_in"), shift=(0, -1)), dict(s_out=ptr("s_in"), shift=(0, 7)),
             dict(l_out=ptr("l_in") + 2), dict(s_out=ptr("s_in") + 4 * 31), dict(l_in=ptr("l_out") + 62)]
    cases += [dict(frame=f) for f in bad_frames] + [dict(map=_c_map(eng, **kw)) for kw in _BAD_MAPS] + [dict(map=_c_map(eng, reserved=k)) for k in range(7)]
    for kw in cases:
        rc, text = call(**kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_occupancy_fuse"), (sorted(kw), rc, text)
    # legal and without work: batch 0, no shift, in place - nothing is enqueued
    assert call(batch=0, l_out=ptr("l_in"), s_out=ptr("s_in")) == 0 and call(batch=0, l_out=ptr("l_in"), s_in=None, s_out=None, state=None, poses=None) == 0
    assert all((b == 0x5A).all() for b in bufs.values())
    assert eng.debug_occupancy_fuse(True, None) == 0


def test_header_build_and_loader_agree(eng):
    """The header declares the map spec's words in the order of the ctypes structure, the library exports the entries the header declares,
    and build.py lists the new sources and header."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct sv_occupancy_map_spec \{(.*?)\} sv_occupancy_map_spec;", src, flags=re.S).group(1)
    words = [w.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for w in decl.split(",")]
    sv_mod = util.pkg("stereo_vision.sv")
    assert words == list(sv_mod.OCCUPANCY_MAP_WORDS) + ["reserved[7]"] == [k for k, _ in eng.SvOccupancyMapSpec._fields_[:-1]] + ["reserved[7]"]
    declared = set(re.findall(r"\(?\b(sv_[a-z_]*occupancy_fuse[a-z_]*)\)?\s*\(", src))
    assert declared == {"sv_occupancy_fuse_device", "sv_debug_occupancy_fuse"}
    L = eng.occupancy_map_lib()
    assert all(hasattr(L, n) for n in declared) and len(L.sv_occupancy_fuse_device.argtypes) == 13
    build = util.pkg("build")
    assert "occupancy_map_kernels.hip" in build.SOURCES and "occupancy_map.cpp" in build.SOURCES and "occupancy_map_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("occupancy_map_kernels.hip", "occupancy_map.cpp", "occupancy_map_kernels.h"))
    assert "occupancy_fuse" in sv_mod.__doc__ and "double-width" in open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()


# ---------------------------------------------------------------------------------------------------------------- GPU

CLI_GRID = dict(x_range=(0, 40), y_range=(-20, 20), z_range=(-1.4, 1.0), scale=10)
DRIVE_MAP = dict(x_range=(-10, 60), y_range=(-30, 30), scale=10)  # 700 x 600 cells, top 600, left 300


def _drive_poses(n):
    b = np.arange(n, dtype=np.float64)
    return np.stack([0.8 * b, 0.05 * b, np.cos(0.03 * b), np.sin(0.03 * b)], -1)


def _gpu(eng, state, poses, frame, words, logodds=None, last_seen=None, seq0=0, shift=(0, 0)):
    """engine.occupancy_fuse on numpy arrays -> dict of numpy arrays."""
    res = eng.occupancy_fuse(_cuda(np.asarray(state, np.uint8)), np.asarray(poses, np.float64), frame, words, None if logodds is None else _cuda(logodds),
                             None if last_seen is None else _cuda(last_seen), seq0, shift)
    return {"logodds": res.logodds.cpu().numpy(), "last_seen": res.last_seen.cpu().numpy()}


def _counted(eng, cull, fn):
    """fn() under sv_debug_occupancy_fuse(cull, counter) -> (its result, the lookups counted)."""
    import torch
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    try:
        assert eng.debug_occupancy_fuse(cull, counter) == 0
        out = fn()
        torch.cuda.synchronize()
    finally:
        eng.debug_occupancy_fuse(True, None)
    return out, int(counter.item())


SMALL = {"9x5": (HAND_FRAME, dict(_GOOD_MAP, top=20, left=13, rows=37, cols=29, scale=2)),
         "41x41": (dict(x_range=(0, 4), y_range=(-2, 2), scale=10), dict(_GOOD_MAP, top=33, left=15, rows=37, cols=29, scale=5))}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SMALL))
def test_smallest_shapes_equal_the_definition(sv, eng, case):
    frame, words = SMALL[case]
    fx, fy, _, frows, fcols = sv.occupancy_frame_grid(frame)
    assert (frows, fcols) == tuple(int(v) for v in case.split("x"))
    cell = 1.0 / words["scale"]
    rng = np.random.default_rng(11)
    kinds = {"identity": IDENTITY, "translation": (0.37 * cell * 3, -1.29 * cell, 1.0, 0.0), "quarter": QUARTER, "yaw": tuple(sv.occupancy_pose(0.3, -0.2, 0.5)),
             "far": (1000.0, 0.0, 1.0, 0.0), "nan": (0.0, NAN, 1.0, 0.0)}
    L0 = rng.integers(-200, 351, (37, 29)).astype(np.int16)
    S0 = rng.integers(-1, 9, (37, 29)).astype(np.int32)
    for name, pose in kinds.items():
        state = rng.integers(0, 4, (1, frows, fcols)).astype(np.uint8)
        want = sv.occupancy_fuse(state, [pose], frame, words, L0, S0, seq0=9)
        got, lookups = _counted(eng, True, lambda: _gpu(eng, state, [pose], frame, words, L0, S0, seq0=9))
        assert _same(got, want), (case, name)
        touched = (want["last_seen"] == 9).any()
        assert touched == (name not in ("far", "nan")), (case, name)
        if name == "far":
            assert lookups == 0
    pool = [kinds[k] for k in ("yaw", "far", "translation", "nan", "quarter", "identity")]
    for B in (1, 3, 5):
        poses = np.array([pool[(b + B) % len(pool)] for b in range(B)])
        state = rng.integers(0, 4, (B, frows, fcols)).astype(np.uint8)
        state[-1, ::3] = 255
        want = sv.occupancy_fuse(state, poses, frame, words, seq0=2)
        assert _same(_gpu(eng, state, poses, frame, words, seq0=2), want), (case, B)
        assert _same(_gpu(eng, state, poses, frame, words, L0, S0, seq0=2, shift=(3, -2)), sv.occupancy_fuse(state, poses, frame, words, L0, S0, seq0=2, shift=(3, -2))), (case, B)
    # no last_seen kept
    res = eng.occupancy_fuse(_cuda(state), poses, frame, words, last_seen=False)
    assert res.last_seen is None and _bits(res.logodds.cpu().numpy(), sv.occupancy_fuse(state, poses, frame, words)["logodds"])


@pytest.fixture(scope="module")
def random_drive(sv, eng):
    """Eight frames of random states on the CLI grid along the drive's poses, the map words and the definition's result, computed once."""
    rng = np.random.default_rng(23)
    state = rng.integers(0, 3, (8, 401, 401)).astype(np.uint8)
    poses = _drive_poses(8)
    words = sv.occupancy_map_params(**DRIVE_MAP)
    assert (words["top"], words["left"], words["rows"], words["cols"]) == (600, 300, 700, 600)
    return state, poses, words, sv.occupancy_fuse(state, poses, CLI_GRID, words)


@pytest.mark.gpu
def test_cull_never_changes_a_result(sv, eng, random_drive):
    state, poses, words, want = random_drive
    on, n_on = _counted(eng, True, lambda: _gpu(eng, state, poses, CLI_GRID, words))
    off, n_off = _counted(eng, False, lambda: _gpu(eng, state, poses, CLI_GRID, words))
    covered = int((want["last_seen"] >= 0).sum())
    print("lookups with / without the cull: %d / %d; cells covered %d of %d" % (n_on, n_off, covered, 700 * 600))
    assert _same(on, want) and _same(off, want)
    assert n_off == 700 * 600 * 8 and 0 < n_on <= n_off
    # a pose whose (c, s) is no rotation, poses far away and large: the cull's margin follows, the bits stay
    odd = np.array([(5.0, 1.0, 3.0, -2.0), (20.0, -3.0, 0.2, 0.1), (1e17, -1e17, np.cos(0.7), np.sin(0.7)), (1e300, 0.0, 0.0, 1.0), (3.0, 2.0, INF, 0.0), (70.0, 0.0, -1.0, 0.0),
                    (30.0, 40.0, 0.0, -1.0), (25.0, 0.0, 1e-3, 1e-3)])
    want_odd = sv.occupancy_fuse(state, odd, CLI_GRID, words)
    assert _same(_gpu(eng, state, odd, CLI_GRID, words), want_odd) and (want_odd["last_seen"] >= 0).any()
    off_odd, _ = _counted(eng, False, lambda: _gpu(eng, state, odd, CLI_GRID, words))
    assert _same(off_odd, want_odd)


def _raw(eng, state, poses, frame, spec, l_in, s_in, l_out, s_out, seq0=0, shift=(0, 0)):
    """The C entry on caller-owned tensors."""
    import torch
    rc = eng.occupancy_map_lib().sv_occupancy_fuse_device(state.data_ptr(), poses.data_ptr(), state.shape[0], seq0, ctypes.byref(frame), ctypes.byref(spec), shift[0], shift[1],
                                                          l_in.data_ptr(), None if s_in is None else s_in.data_ptr(), l_out.data_ptr(), None if s_out is None else s_out.data_ptr(),
                                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, eng.occupancy_map_lib().sv_last_error(None))


@pytest.mark.gpu
def test_buffer_use_and_repeats(sv, eng, random_drive):
    """Out buffers full of 0xA5, in place with a zero shift, out of place with the scroll test's shifts, five repeats: the definition's bits
    every time."""
    import torch
    state, poses, words, want = random_drive
    state, poses = state[:3], poses[:3]
    frame = eng.occupancy_spec(**CLI_GRID)[0]
    t_state, t_poses = _cuda(state), _cuda(poses)
    rng = np.random.default_rng(29)
    L0 = rng.integers(-200, 351, (700, 600)).astype(np.int16)
    S0 = rng.integers(-1, 5, (700, 600)).astype(np.int32)
    for shift in [(0, 0), (3, -2), (-700, 0), (0, 600), (100, 3), (-3, -100000), (2 ** 31 - 1, 0), (1, 1 - 2 ** 31)]:
        spec = eng.occupancy_map_spec(**DRIVE_MAP)
        want_s = sv.occupancy_fuse(state, poses, CLI_GRID, words, L0, S0, seq0=5, shift=shift)
        seen = set()
        for rep in range(5 if shift in ((0, 0), (3, -2)) else 1):
            l_out = torch.full((700, 600, 2), 0xA5, dtype=torch.uint8, device="cuda").view(torch.int16).squeeze(-1)
            s_out = torch.full((700, 600, 4), 0xA5, dtype=torch.uint8, device="cuda").view(torch.int32).squeeze(-1)
            _raw(eng, t_state, t_poses, frame, spec, _cuda(L0), _cuda(S0), l_out, s_out, 5, shift)
            got = {"logodds": l_out.cpu().numpy(), "last_seen": s_out.cpu().numpy()}
            assert _same(got, want_s), (shift, rep)
            seen.add(got["logodds"].tobytes() + got["last_seen"].tobytes())
        assert len(seen) == 1
    # in place with a zero shift, with and without last_seen
    want_0 = sv.occupancy_fuse(state, poses, CLI_GRID, words, L0, S0, seq0=5)
    spec = eng.occupancy_map_spec(**DRIVE_MAP)
    l, s = _cuda(L0), _cuda(S0)
    _raw(eng, t_state, t_poses, frame, spec, l, s, l, s, 5)
    assert _same({"logodds": l.cpu().numpy(), "last_seen": s.cpu().numpy()}, want_0)
    l, s_out = _cuda(L0), torch.full((700, 600), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    _raw(eng, t_state, t_poses, frame, spec, l, None, l, None, 5)
    assert _bits(l.cpu().numpy(), want_0["logodds"]) and (s_out == 0x5A5A5A5A).all()
    # batch 0 with a shift only scrolls
    res = eng.occupancy_fuse(t_state[:0], np.zeros((0, 4)), CLI_GRID, words, _cuda(L0), _cuda(S0), shift=(-7, 11))
    assert _bits(res.logodds.cpu().numpy(), sv.occupancy_scroll(L0, (-7, 11), 0)) and _bits(res.last_seen.cpu().numpy(), sv.occupancy_scroll(S0, (-7, 11), -1))
    # refused on the device as on the host: nothing is written
    with pytest.raises(ValueError):
        eng.occupancy_fuse(t_state, poses, CLI_GRID, words, l, _cuda(S0), shift=(1, 0), out=(l, _cuda(S0)))
    for bad in (dict(state=t_state.int()), dict(state=t_state.cpu()), dict(poses=poses[:2]), dict(poses=t_poses.float()), dict(logodds=l.int()), dict(last_seen=l),
                dict(seq0=-1), dict(shift=(0.5, 0)), dict(map=dict(words, rows=0)), dict(frame_grid=dict(CLI_GRID, scale=0)), dict(frame_grid=dict(CLI_GRID, x_range=(0, 41)))):
        with pytest.raises(ValueError):
            eng.occupancy_fuse(**dict(dict(state=t_state, poses=poses, frame_grid=CLI_GRID, map=words), **bad))


@pytest.mark.gpu
def test_batch_and_stream_order(sv, eng, random_drive):
    """One call with B = 6 equals two calls of 3 and six calls of 1 with seq0 advanced, enqueued back to back on one stream."""
    import torch
    state, poses, words, _ = random_drive
    # occupied everywhere first, so that the clamp is reached and the order shows
    state = np.concatenate([np.full((3, 401, 401), 2, np.uint8), state[:3]])
    poses = np.concatenate([poses[:3], poses[:3]])
    want = sv.occupancy_fuse(state, poses, CLI_GRID, words, seq0=100)
    backwards = sv.occupancy_fuse(state[::-1], poses[::-1], CLI_GRID, words, seq0=100)
    assert (want["logodds"] == 350).any() and not np.array_equal(want["logodds"], backwards["logodds"])
    t_state, t_poses = _cuda(state), _cuda(poses)
    for step in (6, 3, 1):
        res = None
        for b in range(0, 6, step):
            res = eng.occupancy_fuse(t_state[b:b + step], t_poses[b:b + step], CLI_GRID, words, None if res is None else res.logodds, None if res is None else res.last_seen,
                                     seq0=100 + b)
        torch.cuda.synchronize()
        assert _same({"logodds": res.logodds.cpu().numpy(), "last_seen": res.last_seen.cpu().numpy()}, want), step


def _drive_frames(n):
    ls = [util.load_png("kitti0_color_left.png")] + [np.repeat(util.load_png("kitti%d_left.png" % k)[..., None], 3, -1) for k in range(1, n)]
    rs = [util.load_png("kitti0_color_right.png")] + [np.repeat(util.load_png("kitti%d_right.png" % k)[..., None], 3, -1) for k in range(1, n)]
    return np.stack(ls), np.stack(rs)


@pytest.fixture(scope="module")
def drive(sv, eng):
    """The seven committed KITTI frames 0 .. 6 through StereoRig.occupancy in vehicle axes on the CLI grid: the OccupancyResult (device), its
    states as numpy, the poses of the drive and the definition's map."""
    ls, rs = _drive_frames(7)
    rig = util.pkg("rig").StereoRig(W, H)
    try:
        occ = rig.occupancy(_cuda(ls), _cuda(rs), pixel_format="rgb", transform=(sv.CAMERA_TO_VEHICLE, None), **CLI_GRID)
        states = occ.state.cpu().numpy()
    finally:
        rig.close()
    assert (states == 2).any() and (states == 1).any()
    poses = _drive_poses(7)
    words = sv.occupancy_map_params(**DRIVE_MAP)
    return occ, states, poses, words, sv.occupancy_fuse(states, poses, CLI_GRID, words)


@pytest.mark.gpu
def test_the_committed_drive(sv, eng, drive):
    import torch
    occ, states, poses, words, want = drive
    assert (want["logodds"] > 85).any() and (want["logodds"] < -40).any()  # evidence accumulates both ways
    # the C entry
    frame, spec = eng.occupancy_spec(**CLI_GRID)[0], eng.occupancy_map_spec(**DRIVE_MAP)
    l, s = torch.zeros((700, 600), dtype=torch.int16, device="cuda"), torch.full((700, 600), -1, dtype=torch.int32, device="cuda")
    _raw(eng, occ.state, _cuda(poses), frame, spec, l, s, l, s)
    assert _same({"logodds": l.cpu().numpy(), "last_seen": s.cpu().numpy()}, want)
    # the engine, with the result's own spec as the frame grid and the map as a spec structure
    res = eng.occupancy_fuse(occ.state, poses, occ.spec, spec)
    assert _same({"logodds": res.logodds.cpu().numpy(), "last_seen": res.last_seen.cpu().numpy()}, want) and res.spec.top == 600
    # rig.OccupancyMap: four frames, a recenter on the vehicle, three frames
    rigmod = util.pkg("rig")
    rig = rigmod.StereoRig(W, H)
    try:
        world = rig.occupancy_map(**DRIVE_MAP)
    finally:
        rig.close()
    assert isinstance(world, rigmod.OccupancyMap) and world.device.type == "cuda"
    first = eng.OccupancyResult(state=occ.state[:4], spec=occ.spec)
    world.update(first, poses[:4])
    shift = world.recenter(poses[3, 0], poses[3, 1])
    assert shift != (0, 0) and world.seq == 4
    world.update(occ.state[4:], _cuda(poses[4:]), CLI_GRID)
    a = sv.occupancy_fuse(states[:4], poses[:4], CLI_GRID, words)
    b = sv.occupancy_fuse(states[4:], poses[4:], CLI_GRID, world.words, a["logodds"], a["last_seen"], seq0=4, shift=shift)
    assert world.seq == 7 and _same({"logodds": world.logodds.cpu().numpy(), "last_seen": world.last_seen.cpu().numpy()}, b)
    # state: the thresholds applied in numpy
    for kw in (dict(), dict(occupied=170, free=-80)):
        got = world.state(**kw)
        assert got.is_cuda and got.dtype == torch.uint8
        assert _bits(got.cpu().numpy(), sv.occupancy_map_state(b["logodds"], b["last_seen"], kw.get("occupied", 85), kw.get("free", -40)))
    assert len(np.unique(world.state().cpu().numpy())) == 3
    # the same drive on CPU tensors: the same bits
    cpu = rigmod.OccupancyMap(device="cpu", **DRIVE_MAP)
    cpu.update(states[:4], poses[:4], CLI_GRID)
    assert cpu.recenter(poses[3, 0], poses[3, 1]) == shift
    cpu.update(states[4:], poses[4:], CLI_GRID)
    assert _bits(cpu.logodds.numpy(), b["logodds"]) and _bits(cpu.last_seen.numpy(), b["last_seen"])
    world.reset()
    assert world.seq == 0 and not world.logodds.any().item() and (world.last_seen == -1).all().item()


@pytest.mark.gpu
def test_cli_writes_the_map(sv, eng, drive, tmp_path):
    from PIL import Image
    occ, states, poses, words, want = drive
    n = 4
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    ls, rs = _drive_frames(n)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    xyyaw = np.stack([0.8 * np.arange(n), 0.05 * np.arange(n), 0.03 * np.arange(n)], -1)
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("# x y yaw\n" + "".join("%r %r %r\n" % tuple(float(v) for v in row) for row in xyyaw))
    with open(tmp_path / "short.txt", "w") as f:
        f.write("0 0 0\n1 0 0\n")
    out = str(tmp_path / "map.png")
    for bad in (["--occupancy-map", out], ["--batch", "3", "--occupancy-map", out], ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt")],
                ["--batch", "3", "--occupancy-map", out, "--poses", str(tmp_path / "short.txt")], ["--batch", "3", "--occupancy-map", out, "--poses", str(tmp_path / "none.txt")]):
        with pytest.raises(SystemExit):
            sv.main(["-k", str(tmp_path / "kitti")] + bad)
    assert not os.path.exists(out)
    sv.main(["-k", str(tmp_path / "kitti"), "--batch", "3", "--occupancy-map", out, "--poses", str(tmp_path / "poses.txt")])
    # the map covers the trajectory's bounding box plus the reach of the CLI grid: ceil(hypot(40, 20)) = 45 m
    ranges = sv.occupancy_map_cover(xyyaw, sv.CLI_TOP_VIEW["x_range"], sv.CLI_TOP_VIEW["y_range"])
    assert ranges == ((-45, 48), (-45, 46))
    cli_words = sv.occupancy_map_params(ranges[0], ranges[1], 10)
    fused = sv.occupancy_fuse(states[:n], sv.occupancy_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2]), CLI_GRID, cli_words)
    state = sv.occupancy_map_state(fused["logodds"], fused["last_seen"], 85, -40)
    got = np.asarray(Image.open(out))
    assert got.shape == (930, 910) and set(np.unique(got).tolist()) == {0, 127, 255} and np.array_equal(got, sv.OCCUPANCY_PNG[state])
