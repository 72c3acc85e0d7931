"""Stereo visual odometry (group (Z)): the numpy definition of the temporal matches against hand numbers, the sums of a pose round against
a per-match model, the egomotion loop on synthetic scenes with a known motion and on two KITTI pairs, the chain of poses - and the GPU
(engine.flow_match / flow_pose_sums / flow_egomotion, StereoRig.flow / .odometry, the CLI's --odometry) against the definition: shape,
dtype and bits."""
import math
import os

import numpy as np
import pytest

import flow_cases as fc
import util
from flow_cases import IDENTITY, KITTI, PAINTED_WANT, PAINTED_WORDS, SMALL, same
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)

SV_ERR_ARG = -1
KITTI_GUESS = fc.pose_of(np.eye(3), (0.0, 0.0, -1.16))


def _rows(got, b=0):
    n = int(got["counts"][b])
    return [tuple(r) for r in got["matches"][b, :n].tolist()], [tuple(r) for r in got["cost"][b, :n].tolist()]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_painted_pair(sv):
    """The hand numbers of flow_cases.painted: the tie to the lower index (T), the flat patch (F), the stripes (S), the best on the rim (R),
    the first and last admissible row and column (A, L), candidates that would leave the image (L), d_cur invalid at the target (C)."""
    prev, cur, d_prev, d_cur = fc.painted()
    got = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **PAINTED_WORDS)
    assert got["matches"].shape == (1, 16, 6) and got["cost"].shape == (1, 16, 2) and got["counts"].shape == (1,)
    assert all(got[k].dtype == np.int32 for k in fc.FIELDS)
    assert _rows(got) == ([m for m, _ in PAINTED_WANT], [c for _, c in PAINTED_WANT])
    assert (got["matches"][0, 6:] == -1).all() and (got["cost"][0, 6:] == -1).all()  # the rows behind the count
    # without d_cur every d1q is -1 and nothing else changes
    bare = sv.flow_match(prev, cur, d_prev, None, SMALL, **PAINTED_WORDS)
    assert _rows(bare) == ([m[:5] + (-1,) for m, _ in PAINTED_WANT], [c for _, c in PAINTED_WANT])
    # a point whose d_prev is 0, negative, inf or NaN is no point
    u, v = fc.PAINTED_D
    for bad in (0.0, -3.0, np.inf, np.nan, 1e-3):  # 1e-3: floor(16 d + 0.5) = 0
        d = d_prev.copy()
        d[0, v, u] = bad
        assert _rows(sv.flow_match(prev, cur, d, d_cur, SMALL, **PAINTED_WORDS))[0] == [m for m, _ in PAINTED_WANT if m[:2] != (u, v)]
    # one row too few: -1, and the rows are the first five
    short = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, capacity=5))
    assert short["counts"].tolist() == [-1] and short["matches"][0].tolist() == [list(m) for m, _ in PAINTED_WANT[:5]]
    exact = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, capacity=6))
    assert exact["counts"].tolist() == [6]
    # a ratio the tie's 100 against 200 misses, and a max_cost below it
    assert (20, 4) not in [m[:2] for m in _rows(sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, ratio=128)))[0]]
    assert (20, 4) not in [m[:2] for m in _rows(sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, max_cost=99)))[0]]
    assert (20, 4) in [m[:2] for m in _rows(sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, max_cost=100, ratio=129)))[0]]


def test_rim_rule_per_axis(sv):
    """wx = 0 or wy = 0 switches the rim rule off on that axis: C moves by (0, -1) and matches in a window of one column - second (0, +1),
    which holds cur's pixel: 200 -, D moves by (-1, 0) and matches in a window of one row, second (+2, 0): 100.  R's best stays on the
    rim of the one row, and S, whose stripes repeat along a row, is ambiguous only across rows here: (-2, 0) meets the flat column 24,
    five times 40.  In the one column T stays where it is: (0, 0) costs 100 - cur's other pixel -, and (0, +-2), which hold both of
    cur's pixels off the centre, cost 300."""
    prev, cur, d_prev, d_cur = fc.painted()
    col = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, wx=0))
    assert _rows(col) == ([(20, 4, 128, 20, 4, 64), (16, 20, 128, 16, 19, -1)], [(100, 300), (0, 200)])
    row = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, wy=0))
    assert _rows(row) == ([(20, 4, 128, 19, 4, 64), (28, 12, 128, 28, 12, 64), (8, 20, 128, 7, 20, 64)], [(100, 200), (0, 200), (0, 100)])
    none = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, wx=0, wy=0))  # one candidate: never a second
    assert none["counts"].tolist() == [0]


def test_shifted_halves(sv):
    prev, cur, d_prev, d_cur, flows, half = fc.shifted_halves()
    words = dict(step=4, r=3, wx=8, wy=8, capacity=512)
    got = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **words)
    rows, _ = _rows(got)
    H, W = prev.shape[1:]
    lattice = len(range(0, H, 4)) * len(range(0, W, 4))
    assert len(rows) >= lattice // 2
    inside = 0
    for u0, v0, d0q, u1, v1, d1q in rows:
        side = 0 if u0 < half else 1
        x0, x1 = (0, half) if side == 0 else (half, W)
        (dx, dy) = flows[side]
        if x0 <= u0 - 3 and u0 + 3 < x1 and x0 <= u0 + dx - 3 and u0 + dx + 3 < x1 and 0 <= v0 + dy - 3 and v0 + dy + 3 < H:  # both patches inside one half
            assert (u1 - u0, v1 - v0) == (dx, dy), (u0, v0, u1, v1)
            inside += 1
        assert d0q == math.floor(16.0 * float(d_prev[0, v0, u0]) + 0.5) and d1q == (math.floor(16.0 * float(d_cur[0, v1, u1]) + 0.5) if d_cur[0, v1, u1] > 0 else -1)
    assert inside >= lattice // 3


def test_a_guess_with_a_small_window(sv):
    """A constant disparity of 10 px puts every point at z = f b / 10 = 2 m under SMALL; the guess t = (3 z / f, -2 z / f, 0) moves every
    centre by (3, -2), the left half's flow.  A window of +-2 around it finds the matches the window of +-8 finds from the identity where
    both hold them: the best is the same candidate, and the second of the smaller set is no smaller."""
    prev, cur, _, d_cur, flows, half = fc.shifted_halves(seed=9)
    d_prev = np.full(prev.shape, 10.0, np.float32)
    wide = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, step=4, r=3, wx=8, wy=8, capacity=512)
    z = SMALL["f"] * (1.0 / SMALL["q32"]) / 10.0
    guess = fc.pose_of(np.eye(3), (3.0 * z / SMALL["f"], -2.0 * z / SMALL["f"], 0.0))
    near = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, guess[None], step=4, r=3, wx=2, wy=2, capacity=512)
    wide_rows, near_rows = _rows(wide)[0], set(_rows(near)[0])
    held = [m for m in wide_rows if abs(m[3] - m[0] - 3) <= 1 and abs(m[4] - m[1] + 2) <= 1]  # the best inside the small window, off its rim
    assert len(held) >= 40 and all(m in near_rows for m in held)
    assert all((m[3] - m[0], m[4] - m[1]) == flows[0] for m in held if m[0] + 8 < half)
    # under the identity guess - given as a pose - the centres are the points themselves
    assert same(sv.flow_match(prev, cur, d_prev, d_cur, SMALL, IDENTITY[None], step=4, r=3, wx=8, wy=8, capacity=512), wide)


def test_match_arguments(sv):
    prev, cur, d_prev, d_cur = fc.painted()
    for bad in (dict(step=0), dict(r=0), dict(r=8), dict(wx=-1), dict(wx=64, wy=64), dict(ratio=257), dict(ratio=-1), dict(max_cost=-1), dict(capacity=65537),
                dict(r=4, wx=64, wy=51), dict(step=1.5)):
        with pytest.raises(ValueError):
            sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **dict(PAINTED_WORDS, **bad))
    assert sv.flow_window_bytes(4, 64, 24) == 8436 and sv.flow_window_bytes(4, 64, 50) == 16132 and sv.flow_window_bytes(4, 64, 51) > sv.FLOW_WINDOW_BYTES
    for cam in (dict(SMALL, f=0.0), dict(SMALL, q32=-2.0), dict(SMALL, cx=np.nan), {"f": 1.0}):
        with pytest.raises(ValueError):
            sv.flow_match(prev, cur, d_prev, d_cur, cam, **PAINTED_WORDS)
    with pytest.raises(ValueError):
        sv.flow_match(prev, cur[:, :, :-1], d_prev, d_cur, SMALL, **PAINTED_WORDS)
    with pytest.raises(ValueError):
        sv.flow_match(prev, cur, d_prev.astype(np.float64), d_cur, SMALL, **PAINTED_WORDS)
    with pytest.raises(ValueError):
        sv.flow_match(prev, cur, d_prev, d_cur, SMALL, np.zeros((2, 12)), **PAINTED_WORDS)


def test_sums_against_the_model(sv):
    seen = {"inliers": 0, "dinliers": 0, "behind": 0}
    for seed in range(30):
        matches, counts, cam, poses, gate, dgate = fc.random_sums_case(seed)
        got = sv.flow_pose_sums(matches, counts, cam, poses, gate, dgate)
        assert got.shape == (3, 32) and got.dtype == np.int64
        assert np.array_equal(got, sv.flow_pose_sums_brute(matches, counts, cam, poses, gate, dgate)), seed
        assert not got[1].any()  # a count of 0 or -1
        if not np.isfinite(poses[0]).all():
            assert not got[0].any()  # a pose that is not finite keeps nothing
        if gate == 0:
            assert (got[:, 3] == 0).all()
        assert (got[:, 2] <= got[:, 1]).all() and (got[:, 1] <= got[:, 0]).all() and (got[:, 0] <= matches.shape[1]).all()
        seen["inliers"] += int(got[:, 1].sum())
        seen["dinliers"] += int(got[:, 2].sum())
        seen["behind"] += int(((matches[2, :, 2] >= 1) & (matches[2, :, 2] <= 2 ** 20)).sum()) - int(got[2, 0])  # a disparity, and not inside
    assert seen["inliers"] > 500 and seen["dinliers"] > 100 and seen["behind"] > 100
    assert len(sv.FLOW_SUMS) == 32
    for bad in (dict(gate_q=-1), dict(gate_q=2 ** 20 + 1), dict(dgate_q=1.5)):
        with pytest.raises(ValueError):
            sv.flow_pose_sums(matches, counts, cam, poses, **bad)


def test_one_match_by_hand(sv):
    """A point on the axis, 2 m away, seen again one pixel to the right and half a pixel of disparity larger under the identity: with f = 40,
    b = 0.5, cx = 15.5, cy = 11.5 the pixel (15.5, 11.5) is no lattice point, so take u0 = 16, v0 = 12: x = y = 0.5 * 2 / 40 = 0.025."""
    m = np.array([[[16, 12, 160, 17, 12, 168]]], np.int32)  # d0 = 10 px: z = 40 * 0.5 / 10 = 2
    got = sv.flow_pose_sums(m, np.array([1], np.int32), SMALL, IDENTITY[None], 64, 32)[0]
    Ju = [320, 0, -4, 0, 640, -8]      # 16 (f/z, 0, -f x/z^2, -f x y/z^2, f (1 + x^2/z^2), -f y/z) = (320, 0, -4, -0.05, 640.1, -8), rounded
    Jv = [0, 320, -4, -640, 0, 8]
    Jd = [0, 0, -80, -2, 2, 0]         # 16 (0, 0, -f b/z^2, -f b y/z^2, f b x/z^2, 0) = (0, 0, -80, -2, 2, 0)
    ru, rv, rd = 16, 0, 8
    want = [1, 1, 1, 256, 64] + [Ju[i] * ru + Jv[i] * rv + Jd[i] * rd for i in range(6)]
    want += [Ju[i] * Ju[j] + Jv[i] * Jv[j] + Jd[i] * Jd[j] for i in range(6) for j in range(i, 6)]
    assert got.tolist() == want
    tight = sv.flow_pose_sums(m, np.array([1], np.int32), SMALL, IDENTITY[None], 15, 32)[0]
    assert tight.tolist() == [1] + [0] * 31
    no_d = sv.flow_pose_sums(m, np.array([1], np.int32), SMALL, IDENTITY[None], 16, 7)[0]
    assert no_d[:5].tolist() == [1, 1, 0, 256, 0] and no_d[5:11].tolist() == [Ju[i] * ru for i in range(6)]


@pytest.mark.parametrize("seed", range(4))
def test_synthetic_egomotion(sv, seed):
    """1500 matches, whole-pixel targets, 20 % outliers, 30 % without d1, identity start, default gates.  Measured with this definition:
    0.31 .. 0.47 mm and 0.0011 .. 0.0020 degrees over the four seeds, the inliers equal to the true count."""
    matches, counts, pose = fc.scene_of(seed)
    got = sv.flow_egomotion(matches, counts, KITTI)
    t_err = float(np.abs(got["poses"][0, 9:] - pose[9:]).max())
    r_err = fc.angle_between(got["poses"][0, :9], pose[:9])
    truth = int(sv.flow_pose_sums(matches, counts, KITTI, pose[None], 48, 32)[0, 1])  # the matches within the last gate, 3 px, of the true motion
    print("seed %d: %d rounds, |t - t_true| = %.3f mm, rotation error %.5f deg, inliers %d of %d true" % (seed, got["rounds"], 1000 * t_err, r_err, got["inliers"][-1, 0], truth))
    assert got["ok"].all() and 5 <= got["rounds"] <= 10
    assert t_err <= 2e-3 and r_err <= 0.01
    assert abs(int(got["inliers"][-1, 0]) - truth) <= truth // 100
    assert got["inliers"].shape == (got["rounds"], 1) and got["rms_px"].shape == (got["rounds"], 1) and got["sums"].shape == (1, 32)
    assert got["rms_px"][-1, 0] < 1.0 < got["rms_px"][0, 0]


def test_egomotion_edges(sv):
    matches, counts, pose = fc.scene_of(0, 40)
    few = sv.flow_egomotion(matches[:, :8], np.array([8], np.int32), KITTI)  # fewer than min_inliers: not ok, the start kept
    assert not few["ok"].any() and np.array_equal(few["poses"][0], IDENTITY)
    none = sv.flow_egomotion(matches, np.array([-1], np.int32), KITTI, start=pose[None])
    assert not none["ok"].any() and np.array_equal(none["poses"][0], pose)
    assert sv.flow_egomotion(matches, counts, KITTI, iterations=0)["rounds"] == 0
    with pytest.raises(ValueError):
        sv.flow_egomotion(matches, counts, KITTI, gates=())
    with pytest.raises(ValueError):
        sv.flow_egomotion(matches, counts, KITTI, eps=(1.0,))


def test_chain(sv):
    start = fc.pose_of(fc.rotation(0.01, -0.02, 0.3), (5.0, -2.0, 0.5))
    same_place = sv.flow_chain(np.tile(IDENTITY, (3, 1)), start)
    assert same_place.shape == (4, 12) and all(np.array_equal(p, start) for p in same_place)
    # a known motion and its inverse
    R, t = fc.rotation(0.004, -0.015, 0.002), np.array([0.02, -0.01, -1.17])
    back = fc.pose_of(R.T, -R.T @ t)
    there = sv.flow_chain(np.stack([fc.pose_of(R, t), back]), start)
    assert np.abs(there[2] - start).max() <= 1e-12 and np.abs(there[1] - start).max() > 1.0
    # the camera looks along the vehicle's x: the points come 1.17 m nearer, the frame moves 1.17 m forward
    fwd = sv.flow_chain(np.tile(fc.pose_of(np.eye(3), (0.0, 0.0, -1.17)), (2, 1)), None, sv.CAMERA_TO_VEHICLE, None)
    assert np.abs(fwd[:, 9:] - np.array([[0, 0, 0], [1.17, 0, 0], [2.34, 0, 0]])).max() <= 1e-12 and np.abs(fwd[:, :9] - IDENTITY[:9]).max() <= 1e-15
    # with a lever arm: a yaw of the camera about its y axis (down) turns the vehicle clockwise about z
    turn = sv.flow_chain(fc.pose_of(fc.rotation(0.0, 0.1, 0.0), (0, 0, 0))[None], None, sv.CAMERA_TO_VEHICLE, np.array([1.0, 0.0, 1.5]))
    assert abs(math.atan2(turn[1, 3], turn[1, 0]) - 0.1) <= 1e-12
    # a motion that is not ok repeats the one before it, the first the identity
    rel = np.stack([fc.pose_of(np.eye(3), (0, 0, -1.0)), fc.pose_of(np.eye(3), (0, 0, -9.0)), fc.pose_of(np.eye(3), (0, 0, -2.0))])
    held = sv.flow_chain(rel, None, sv.CAMERA_TO_VEHICLE, None, ok=[True, False, True])
    assert np.abs(held[:, 9] - np.array([0.0, 1.0, 2.0, 4.0])).max() <= 1e-12
    first = sv.flow_chain(rel, None, sv.CAMERA_TO_VEHICLE, None, ok=[False, True, True])
    assert np.abs(first[:, 9] - np.array([0.0, 0.0, 9.0, 11.0])).max() <= 1e-12
    assert sv.flow_pose_lines(fwd)[1] == "1.17 0.0 0.0"


@pytest.fixture(scope="module")
def kitti_d1():
    """D1 of kitti0 .. kitti2 from the oracle on the CPU at disp_max = 127, with the left images."""
    from pyoracle import ElasParams, Oracle
    L = [util.load_png("kitti%d_left.png" % k) for k in range(3)]
    R = [util.load_png("kitti%d_right.png" % k) for k in range(3)]
    return L, [Oracle().process(ElasParams.driver(127), l, r)[0] for l, r in zip(L, R)]


def _in_the_band(pose, inliers, matches):
    """The motion band of the committed KITTI drive: 11.6 m/s at 10 Hz, straight."""
    t, angle = pose[9:], fc.angle_between(pose[:9], np.eye(3))
    return matches >= 500 and inliers >= 0.8 * matches and -1.25 <= t[2] <= -1.08 and abs(t[0]) < 0.05 and abs(t[1]) < 0.05 and angle < 0.5


@pytest.mark.parametrize("k", [0, 1])
def test_kitti_pair(sv, kitti_d1, k):
    """kitti k -> k + 1 at step 16 under a guess of 1.16 m forward.  Measured: 698 and 757 matches, 619 and 667 inliers, t = (-0.007, -0.006,
    -1.153) and (0.003, -0.004, -1.167) m, 0.11 and 0.21 degrees."""
    L, D = kitti_d1
    m = sv.flow_match(L[k][None], L[k + 1][None], D[k][None], D[k + 1][None], KITTI, KITTI_GUESS[None], step=16, r=4, wx=8, wy=8, capacity=4096)
    got = sv.flow_egomotion(m["matches"], m["counts"], KITTI, KITTI_GUESS[None])
    print("kitti%d->%d: %d matches, %d inliers, t = %s, %.3f deg" % (k, k + 1, m["counts"][0], got["inliers"][-1, 0], got["poses"][0, 9:], fc.angle_between(got["poses"][0, :9], np.eye(3))))
    assert got["ok"].all() and _in_the_band(got["poses"][0], int(got["inliers"][-1, 0]), int(m["counts"][0]))


def test_odometry_driver(sv):
    """flow_odometry's three kinds of guess, with callables that record what they were asked for."""
    asked = []

    def match_of(lo, hi, g, wx, wy):
        asked.append((lo, hi, None if g is None else g.copy(), wx, wy))
        return {"lo": lo}

    def ego_of(got, start):
        n = len(start)
        ok = np.array([got["lo"] != 1] * n)  # pair 1 fails
        return {"poses": start + 1.0, "ok": ok, "rounds": 2, "inliers": np.full((2, n), 7)}

    got = sv.flow_odometry(match_of, ego_of, 4, "velocity", cold=(9, 5), wx=3, wy=2)
    assert [(a[0], a[1], a[3], a[4]) for a in asked] == [(0, 1, 9, 5), (1, 2, 3, 2), (2, 3, 9, 5), (3, 4, 3, 2)]
    assert asked[0][2] is None and np.array_equal(asked[1][2], got["rel"][0:1]) and asked[2][2] is None and np.array_equal(asked[3][2], got["rel"][2:3])
    assert got["ok"].tolist() == [True, False, True, True] and got["inliers"].tolist() == [7] * 4 and len(got["calls"]) == 4
    del asked[:]
    sv.flow_odometry(match_of, ego_of, 3, "identity", cold=(9, 5))
    sv.flow_odometry(match_of, ego_of, 3, np.tile(IDENTITY, (3, 1)))
    sv.flow_odometry(match_of, ego_of, 2, "velocity", first=KITTI_GUESS)
    assert [(a[0], a[1], a[2] is None, a[3], a[4]) for a in asked] == [(0, 3, True, 9, 5), (0, 3, False, 8, 8), (0, 1, False, 8, 8), (1, 2, False, 8, 8)]
    assert sv.flow_odometry(match_of, ego_of, 0)["rel"].shape == (0, 12)
    for bad in (dict(guess="speed"), dict(guess=np.zeros((2, 12))), dict(window=3)):
        with pytest.raises(ValueError):
            sv.flow_odometry(match_of, ego_of, 3, **bad)


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    for name in ("sv_flow_match_workspace", "sv_flow_match_device", "sv_flow_pose_sums_workspace", "sv_flow_pose_sums_device", "sv_flow_spec"):
        assert name in text
    assert "(Z) Behind the engine" in text and text.index("/* ---- (Z)") < text.index("/* ---- (A)")
    build = util.pkg("build")
    assert "flow_kernels.hip" in build.SOURCES and "flow.cpp" in build.SOURCES and "flow_kernels.h" in build.HEADERS
    assert set(util.pkg("engine").STAGE_SIGNATURES["flow"]) == {"sv_flow_match_workspace", "sv_flow_match_device", "sv_flow_pose_sums_workspace", "sv_flow_pose_sums_device"}
    with pytest.raises(SystemExit):
        sv.main(["-k", "nowhere", "--odometry", "poses.txt"])  # needs --batch


# ---------------------------------------------------------------------------------------------------------------- GPU

def _gpu_match(eng, prev, cur, d_prev, d_cur, cam, guess=None, **words):
    res = eng.flow_match(_cuda(prev), _cuda(cur), _cuda(d_prev), None if d_cur is None else _cuda(d_cur), cam, guess, **words)
    return {k: getattr(res, k).cpu().numpy() for k in fc.FIELDS}


@pytest.mark.gpu
def test_gpu_painted_and_shifted(sv, eng):
    prev, cur, d_prev, d_cur = fc.painted()
    for words in (PAINTED_WORDS, dict(PAINTED_WORDS, capacity=5), dict(PAINTED_WORDS, wx=0), dict(PAINTED_WORDS, wy=0), dict(PAINTED_WORDS, wx=0, wy=0),
                  dict(PAINTED_WORDS, capacity=0)):
        assert same(_gpu_match(eng, prev, cur, d_prev, d_cur, SMALL, **words), sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **words)), words
    assert same(_gpu_match(eng, prev, cur, d_prev, None, SMALL, **PAINTED_WORDS), sv.flow_match(prev, cur, d_prev, None, SMALL, **PAINTED_WORDS))
    prev, cur, d_prev, d_cur, _, _ = fc.shifted_halves()
    words = dict(step=4, r=3, wx=8, wy=8, capacity=512)
    want = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, **words)
    assert want["counts"][0] > 100 and same(_gpu_match(eng, prev, cur, d_prev, d_cur, SMALL, **words), want)
    guess = fc.pose_of(fc.rotation(0.01, -0.02, 0.005), (0.05, -0.02, -0.1))[None]
    assert same(_gpu_match(eng, prev, cur, d_prev, d_cur, SMALL, guess, **words), sv.flow_match(prev, cur, d_prev, d_cur, SMALL, guess, **words))


@pytest.fixture(scope="module")
def odd_pair():
    """40 x 67: W is no multiple of 4, so the window rows start at every byte alignment; a smooth texture, so that neighbouring candidates
    cost nearly the same and the best's neighbours are their lanes' least."""
    prev = fc.texture(21, 40, 67, smooth=2)
    cur = np.roll(prev, (1, -2), (0, 1))
    cur[::7, ::5] += 3
    rng = np.random.default_rng(22)
    d_prev = rng.uniform(0.5, 40.0, (40, 67)).astype(np.float32)
    d_prev[rng.random((40, 67)) < 0.1] = np.nan
    d_cur = rng.uniform(-2.0, 40.0, (40, 67)).astype(np.float32)
    return prev[None], cur[None], d_prev[None], d_cur[None]


@pytest.mark.gpu
@pytest.mark.parametrize("r", [1, 2, 4, 7])
def test_gpu_odd_width(sv, eng, odd_pair, r):
    cam = dict(SMALL, cx=33.0, cy=19.5)
    guess = fc.pose_of(fc.rotation(0.002, 0.004, -0.01), (0.01, 0.0, -0.05))[None]
    for wx, wy in ((0, 0), (3, 2), (8, 8), (15, 3), (31, 2), (32, 1)):  # 2 wx + 1 = 31, 63, 65: two of the best's neighbours in one lane
        words = dict(step=5, r=r, wx=wx, wy=wy, ratio=250, capacity=128)
        for g in (None, guess):
            want = sv.flow_match(*odd_pair, cam, g, **words)
            assert same(_gpu_match(eng, *odd_pair, cam, g, **words), want), (words, g is None)
        assert (wx, wy) == (0, 0) or want["counts"][0] > 5


@pytest.mark.gpu
def test_gpu_window_at_the_lds_limit(sv, eng, odd_pair):
    cam = dict(SMALL, cx=33.0, cy=19.5)
    words = dict(step=9, r=4, wx=64, wy=50, ratio=250, capacity=64)  # 16132 bytes a wavefront
    assert same(_gpu_match(eng, *odd_pair, cam, **words), sv.flow_match(*odd_pair, cam, **words))
    L = eng.flow_lib()
    import ctypes
    need = ctypes.c_size_t(77)
    spec = eng.flow_spec(cam, **words)
    assert L.sv_flow_match_workspace(67, 40, 1, ctypes.byref(spec), ctypes.byref(need)) == 0 and need.value == 8 * 5 * 32
    spec.wy = 51  # 16428 bytes: refused by the workspace call and by the launch
    need.value = 77
    assert L.sv_flow_match_workspace(67, 40, 1, ctypes.byref(spec), ctypes.byref(need)) == SV_ERR_ARG and need.value == 77
    assert b"LDS" in L.sv_last_error(None)
    with pytest.raises(ValueError):
        _gpu_match(eng, *odd_pair, cam, **dict(words, wy=51))


@pytest.mark.gpu
def test_gpu_batch_of_three(sv, eng):
    """Three frames with different counts: the shifted halves, a frame without a valid disparity, and the halves again at another seed with
    more matches than the capacity."""
    a, b = fc.shifted_halves(5), fc.shifted_halves(6)
    prev, cur = np.concatenate([a[0], a[0], b[0]]), np.concatenate([a[1], a[1], b[1]])
    d_prev, d_cur = np.concatenate([a[2], np.full_like(a[2], -1.0), np.abs(b[2])]), np.concatenate([a[3], a[3], b[3]])
    guess = np.stack([IDENTITY, IDENTITY, fc.pose_of(np.eye(3), (0.01, 0.0, 0.0))])
    for g in (None, guess):
        words = dict(step=4, r=2, wx=6, wy=4, capacity=224)  # 212 matches in frame 0, 236 in frame 2
        want = sv.flow_match(prev, cur, d_prev, d_cur, SMALL, g, **words)
        assert want["counts"][1] == 0 and (g is not None or (0 < want["counts"][0] < 224 and want["counts"][2] == -1))
        assert same(_gpu_match(eng, prev, cur, d_prev, d_cur, SMALL, g, **words), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 700])
def test_gpu_sums_at_chunk_edges(sv, eng, n):
    m0, _, pose = fc.scene_of(1, max(n, 1))
    m1, _, _ = fc.scene(77, max(n, 1), t=(0.0, 0.0, -5.0))  # many points behind the camera
    matches = np.ascontiguousarray(np.concatenate([m0, m1])[:, :n])
    counts = np.array([n, max(n - 3, 0)], np.int32)
    poses = np.stack([pose, IDENTITY])
    for gate, dgate in ((None, None), (48, 32), (0, 0)):
        want = sv.flow_pose_sums(matches, counts, KITTI, poses, gate, dgate)
        got = eng.flow_pose_sums(_cuda(matches), _cuda(counts), KITTI, poses, gate, dgate).cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want), (n, gate)
    assert n == 0 or want[0, 0] > 0


@pytest.mark.gpu
def test_gpu_sums_on_the_random_cases(sv, eng):
    for seed in range(30):
        matches, counts, cam, poses, gate, dgate = fc.random_sums_case(seed)
        got = eng.flow_pose_sums(_cuda(matches), _cuda(counts), cam, _cuda(poses), gate, dgate).cpu().numpy()
        assert np.array_equal(got, sv.flow_pose_sums(matches, counts, cam, poses, gate, dgate)), seed


@pytest.mark.gpu
def test_gpu_egomotion_equals_the_definition(sv, eng):
    scenes = [fc.scene_of(seed) for seed in range(4)]
    matches, counts = np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])
    want = sv.flow_egomotion(matches, counts, KITTI)
    got = eng.flow_egomotion(_cuda(matches), _cuda(counts), KITTI)
    assert got.rounds == want["rounds"] and got.poses.tobytes() == want["poses"].tobytes() and np.array_equal(got.ok, want["ok"])
    assert np.array_equal(got.inliers, want["inliers"]) and got.rms_px.tobytes() == want["rms_px"].tobytes() and np.array_equal(got.sums.cpu().numpy(), want["sums"])
    for s, p in zip(scenes, got.poses):
        assert np.abs(p[9:] - s[2][9:]).max() <= 2e-3 and fc.angle_between(p[:9], s[2][:9]) <= 0.01


@pytest.mark.gpu
def test_gpu_argument_checks(eng):
    import ctypes
    import torch
    L = eng.flow_lib()
    good = eng.flow_spec(SMALL, **PAINTED_WORDS)
    buf = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    need = ctypes.c_size_t()

    def match(spec=good, prev=p, counts=p, ws=p, ws_bytes=32768, batch=1, w=32, h=24, guess=None, matches=p):
        return L.sv_flow_match_device(prev, p, p, None, guess, batch, w, h, ctypes.byref(spec), matches, p, counts, ws, ws_bytes, None)

    def sums(spec=good, batch=1, cap=16, gate=16, dgate=16, out=p, ws=p, ws_bytes=32768, poses=p):
        return L.sv_flow_pose_sums_device(p, p, poses, batch, cap, ctypes.byref(spec), gate, dgate, out, ws, ws_bytes, None)

    assert match() == 0 and sums() == 0 and match(batch=0, prev=None, counts=None, ws=None, ws_bytes=0) == 0
    for field, bad in (("step", 0), ("r", 0), ("r", 8), ("wx", -1), ("wy", 8193), ("ratio", 257), ("max_cost", -1), ("capacity", 65537), ("f", 0.0), ("b16", float("nan")),
                       ("fb", -1.0), ("cx", float("inf"))):
        spec = eng.flow_spec(SMALL, **PAINTED_WORDS)
        setattr(spec, field, bad)
        assert match(spec=spec) == SV_ERR_ARG, field
        assert L.sv_flow_match_workspace(32, 24, 1, ctypes.byref(spec), ctypes.byref(need)) == SV_ERR_ARG, field
    spec = eng.flow_spec(SMALL, **PAINTED_WORDS)
    spec.reserved[3] = 1
    assert match(spec=spec) == SV_ERR_ARG and sums(spec=spec) == SV_ERR_ARG
    spec = eng.flow_spec(SMALL, **PAINTED_WORDS)
    spec.wx, spec.wy = 64, 64  # 16641 candidates
    assert match(spec=spec) == SV_ERR_ARG
    for kw in (dict(prev=None), dict(counts=None), dict(ws=None), dict(ws_bytes=8 * 6 * 32 - 1), dict(batch=-1), dict(batch=65536), dict(w=0), dict(h=8193),
               dict(guess=p + 4), dict(matches=None), dict(matches=p + 2), dict(ws=p + 2)):
        assert match(**kw) == SV_ERR_ARG, kw
    assert L.sv_flow_match_workspace(32, 24, 1, ctypes.byref(good), None) == SV_ERR_ARG
    for kw in (dict(batch=-1), dict(batch=65536), dict(cap=-1), dict(cap=65537), dict(gate=-1), dict(gate=2 ** 20 + 1), dict(dgate=-1), dict(out=None), dict(out=p + 4),
               dict(ws=None), dict(ws=p + 4), dict(ws_bytes=255), dict(poses=None), dict(poses=p + 4)):
        assert sums(**kw) == SV_ERR_ARG, kw
    assert L.sv_flow_pose_sums_workspace(16, 1, None) == SV_ERR_ARG and L.sv_flow_pose_sums_workspace(65537, 1, ctypes.byref(need)) == SV_ERR_ARG
    assert L.sv_flow_pose_sums_workspace(700, 3, ctypes.byref(need)) == 0 and need.value == 3 * 3 * 32 * 8
    torch.cuda.synchronize()


ODOMETRY_SPEC = dict(step=16, capacity=2048, first=KITTI_GUESS)  # the CPU test's settings: every pair under a guess, windows of +-8
COLD_SPEC = dict(step=16, capacity=2048, cold=(32, 16))          # the first pair from the identity


@pytest.fixture(scope="module")
def kitti_odometry(sv, eng, tmp_path_factory):
    """kitti0 .. kitti3 at full size through StereoRig.odometry, as CUDA tensors and as numpy arrays, with the engine's own D1 and left
    images."""
    import torch
    ls = np.stack([np.repeat(util.load_png("kitti%d_left.png" % k)[..., None], 3, -1) for k in range(4)])
    rs = np.stack([np.repeat(util.load_png("kitti%d_right.png" % k)[..., None], 3, -1) for k in range(4)])
    yml = str(tmp_path_factory.mktemp("flow") / "rectified.yml")
    with open(yml, "w") as f:
        f.write(fc.RECTIFIED_YML)
    rig = util.pkg("rig").StereoRig(1242, 375, calibration=yml, params=eng.SvParams.driver(127))
    try:
        cuda = rig.odometry(torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda(), transform=(sv.CAMERA_TO_VEHICLE, None), **ODOMETRY_SPEC)
        host = rig.odometry(ls, rs, transform=(sv.CAMERA_TO_VEHICLE, None), **ODOMETRY_SPEC)
        cold = rig.odometry(ls[:2], rs[:2], **COLD_SPEC)
        gl, _ = rig.frontend(ls, rs)
        d1 = rig.disparity(ls, rs)
        flow = rig.flow(ls, rs, guess=np.tile(KITTI_GUESS, (3, 1)), step=16, capacity=2048)
        camera = rig.render_camera(1.0)
    finally:
        rig.close()
    return cuda, host, gl, d1, camera, flow, cold


@pytest.mark.gpu
def test_gpu_rig_odometry(sv, kitti_odometry):
    cuda, host, gl, d1, camera, flow, cold = kitti_odometry

    def match_of(lo, hi, g, wx, wy):
        return sv.flow_match(gl[lo:hi], gl[lo + 1:hi + 1], d1[lo:hi], d1[lo + 1:hi + 1], camera, g, step=16, wx=wx, wy=wy, capacity=2048)

    want = sv.flow_odometry(match_of, lambda got, at: sv.flow_egomotion(got["matches"], got["counts"], camera, at), 3, "velocity", **ODOMETRY_SPEC)
    poses = sv.flow_chain(want["rel"], None, sv.CAMERA_TO_VEHICLE, None, want["ok"])
    for got in (cuda, host):
        assert got["rel"].tobytes() == want["rel"].tobytes() and got["poses"].tobytes() == poses.tobytes() and got["poses"].shape == (4, 12)
        assert np.array_equal(got["ok"], want["ok"]) and np.array_equal(got["inliers"], want["inliers"])
        m = {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in got["matches"].items()}
        assert same(m, {k: np.concatenate([c[k] for c in want["calls"]]) for k in fc.FIELDS})
    assert isinstance(host["matches"]["matches"], np.ndarray) and not isinstance(cuda["matches"]["matches"], np.ndarray)
    for k in range(3):
        print("kitti%d->%d: %d matches, %d inliers, t = %s" % (k, k + 1, want["calls"][k]["counts"][0], want["inliers"][k], want["rel"][k, 9:]))
        assert want["ok"][k] and _in_the_band(want["rel"][k], int(want["inliers"][k]), int(want["calls"][k]["counts"][0]))
    assert 3.2 < poses[3, 9] < 3.8 and np.abs(poses[3, 10:]).max() < 0.15  # about 3.5 m forward
    # the cold start: kitti0 -> 1 from the identity over +-32 x +-16.  More of its matches are wrong - the share of inliers is printed, not
    # held against the band, which is the guessed window's -, the motion is the same
    want = sv.flow_odometry(match_of, lambda got, at: sv.flow_egomotion(got["matches"], got["counts"], camera, at), 1, "velocity", **COLD_SPEC)
    assert cold["rel"].tobytes() == want["rel"].tobytes() and np.array_equal(cold["inliers"], want["inliers"]) and cold["ok"].all()
    assert same(cold["matches"], want["calls"][0]) and cold["poses"].tobytes() == sv.flow_chain(want["rel"]).tobytes()
    print("cold: %d matches, %d inliers, t = %s" % (want["calls"][0]["counts"][0], want["inliers"][0], want["rel"][0, 9:]))
    assert _in_the_band(want["rel"][0], 500, 500) and want["calls"][0]["counts"][0] >= 500
    # flow(): the three pairs in one call under a caller's guess
    assert same(flow, sv.flow_match(gl[:-1], gl[1:], d1[:-1], d1[1:], camera, np.tile(KITTI_GUESS, (3, 1)), step=16, capacity=2048))


@pytest.mark.gpu
def test_gpu_cli(sv, eng, tmp_path):
    from PIL import Image
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    for i in range(3):
        for sub, side in (("image_02", "left"), ("image_03", "right")):
            Image.fromarray(np.repeat(util.load_png("kitti%d_%s.png" % (i, side))[..., None], 3, -1)).save(tmp_path / "kitti" / sub / ("%010d.png" % i))
    poses, ply, yml = str(tmp_path / "odo.txt"), str(tmp_path / "ply"), str(tmp_path / "rectified.yml")
    with open(yml, "w") as f:
        f.write(fc.RECTIFIED_YML)
    base = ["-k", str(tmp_path / "kitti"), "--camera_calibration", yml, "--batch", "3"]
    sv.main(base + ["--odometry", poses])
    rows = sv.read_poses(poses, 3)  # what --poses reads
    assert rows[0].tolist() == [0.0, 0.0, 0.0] and 1.0 < rows[1, 0] < 1.3 and 2.1 < rows[2, 0] < 2.5 and np.abs(rows[:, 1:]).max() < 0.1
    rel = np.array([[float(w) for w in line.split()] for line in open(poses + ".rel.txt")])
    assert rel.shape == (2, 12) and all(-1.25 <= t <= -1.08 for t in rel[:, 11])
    chained = sv.flow_chain(rel, None, sv.CAMERA_TO_VEHICLE, None)
    assert [line.split() for line in sv.flow_pose_lines(chained)] == [line.split() for line in open(poses)]
    # two batches overlap by a frame and give the same file
    again = str(tmp_path / "again.txt")
    sv.main(["-k", str(tmp_path / "kitti"), "--camera_calibration", yml, "--batch", "2", "--odometry", again])
    assert open(again).read() == open(poses).read() and open(again + ".rel.txt").read() == open(poses + ".rel.txt").read()
    # the voxel map along the odometry equals the one along the same poses given through --poses
    own, given = str(tmp_path / "own.ply"), str(tmp_path / "given.ply")
    sv.main(base + ["--ply", ply, "--voxel", "0.2", "--voxel-map", own, "--odometry", str(tmp_path / "own.txt")])
    sv.main(base + ["--ply", ply, "--voxel", "0.2", "--voxel-map", given, "--poses", poses])
    assert open(str(tmp_path / "own.txt")).read() == open(poses).read()
    assert open(own, "rb").read() == open(given, "rb").read() and os.path.getsize(own) > 100000
