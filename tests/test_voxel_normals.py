"""The surface normals of the voxel map and point-to-plane alignment (group (Y)): the numpy definitions against hand numbers and against
loops in Python ints and fractions, the accuracy of the table search against an eigen-solver, the fit and the loop on a street, and the
GPU (engine.voxel_map_normals / voxel_map_align_plane_sums / voxel_map_align, rig.VoxelMap.normals / .align, the CLI) against the
definitions - shape, dtype and bits."""
import os
import re

import numpy as np
import pytest

import util
import voxel_align_cases as acases
import voxel_map_cases as cases
import voxel_match_cases as mcases
import voxel_normal_cases as ncases
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_align_cases import HAND, define, key_of
from voxel_map_cases import BOX16, IDENTITY, PROBE_BOX
from voxel_match_cases import shifted
from voxel_normal_cases import AXES, NORMAL_FIELDS, PLANE_FIELDS, same

SV_ERR_ARG = -1
BOX4K = dict(BOX16, capacity=4096)
ZERO = np.zeros((1, 3), np.int32)


def _normals_agree(sv, state, dirs, **kw):
    got = sv.voxel_map_normals(state, dirs, **kw)
    assert same(got, sv.voxel_map_normals_brute(state, dirs, **kw), NORMAL_FIELDS), kw
    E = len(state["key"])
    assert got["normal"].shape == (E,) and got["fit"].shape == (E, 4) and got["counts"].shape == (4,) and got["counts"][3] == 0
    assert got["counts"][2] == (got["normal"] >= 0).sum() and got["counts"][0] >= got["counts"][1] >= got["counts"][2]
    return got


def _planes_agree(sv, state, frame, poses, origin, normal, dirs, **kw):
    got = sv.voxel_map_align_plane_sums(state, *frame, poses, origin, normal, dirs, **kw)
    assert same(got, sv.voxel_map_align_plane_sums_brute(state, *frame, poses, origin, normal, dirs, **kw), PLANE_FIELDS), kw
    point = sv.voxel_map_align_sums(state, *frame, poses, origin, **kw)  # the rows, the pairs and the per-row words are (X)'s
    assert np.array_equal(got["sums"][:, :2], point["sums"][:, :2]) and np.array_equal(got["pair_key"], point["pair_key"]) and np.array_equal(got["pair_d2"], point["pair_d2"])
    return got


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_the_table_of_directions(sv):
    d = sv.voxel_normal_dirs()
    assert d.shape == (513, 4) and d.dtype == np.int8 and not d[:, 3].any()
    assert d[0].tolist() == [127, 0, 0, 0] and d[-1].tolist() == [0, 0, 127, 0] and d[1].tolist() == [-127, 8, 0, 0]  # sorted by (z, y, x)
    s = (d[:, :3].astype(np.int64) ** 2).sum(1)
    assert s.min() == 15972 and s.max() == 16265  # one length within 2 %
    for m in (1, 2, 7, 45):
        t = sv.voxel_normal_dirs(m, 100)
        assert t.shape == (2 * m * m + 1, 4)
        v = t[:, :3].astype(np.int64)
        assert len({tuple(r) for r in v.tolist()} | {tuple(r) for r in (-v).tolist()}) == 2 * len(v)  # no direction twice, nor its opposite
        assert (np.abs(np.sqrt((v * v).sum(1)) - 100.0) < 1.0).all()
    assert sv.voxel_normal_dirs(1).tolist() == [[127, 0, 0, 0], [0, 127, 0, 0], [0, 0, 127, 0]]
    for kw in (dict(m=0), dict(m=46), dict(m=1.5), dict(m=True), dict(radius=0), dict(radius=128)):
        with pytest.raises(ValueError):
            sv.voxel_normal_dirs(**kw)
    unit = sv.voxel_normal_vectors(d, np.array([[0, 512], [-1, 513]]))
    assert unit.shape == (2, 2, 3) and unit[0].tolist() == [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]] and not unit[1].any()
    assert np.abs(np.linalg.norm(sv.voxel_normal_vectors(d, np.arange(513)), axis=1) - 1.0).max() < 1e-12


def test_hand_normals(sv):
    d = sv.voxel_normal_dirs()
    params, calls = ncases.plate_case()
    state = define(sv, params, calls)
    got = _normals_agree(sv, state, d)
    centre, corner, edge = (ncases.entry_of(state, c) for c in ((5, 5, 5), (4, 4, 5), (4, 5, 5)))
    C00 = 9 * 6 * 256 ** 2  # N s2: six of the nine are 256 away on the axis, s1 = 0
    assert got["fit"][centre].tolist() == [9, C00, C00, 0] and got["normal"][centre] == 512 and d[512].tolist() == [0, 0, 127, 0]
    assert got["fit"][corner, 0] == 4 and got["normal"][corner] == -1  # N = 4 < min_nb
    assert got["fit"][edge, 0] == 6 and got["normal"][edge] == 512
    assert got["counts"].tolist() == [9, 5, 5, 0] and got["key"].tolist() == sorted(state["key"].tolist())
    assert (_normals_agree(sv, state, d, min_nb=3)["normal"] == 512).all()
    params, calls = ncases.column_case()
    state = define(sv, params, calls)
    got = _normals_agree(sv, state, d, min_nb=3)
    mid = ncases.entry_of(state, (5, 5, 5))
    assert got["fit"][mid].tolist() == [3, 3 * 2 * 256 ** 2, 0, 0] and (got["normal"] == -1).all() and got["counts"].tolist() == [5, 3, 0, 0]  # lam2 = 0; the two ends have N = 2
    state = define(sv, BOX16, ncases.one_voxel_each([ncases.at_sub((5, 5, 5), (1, 2, 3))]))
    got = _normals_agree(sv, state, d, min_nb=3)
    assert got["fit"].tolist() == [[1, 0, 0, 0]] and got["normal"].tolist() == [-1]  # C = 0, every Q = 0, best = worst = 0
    # tables: an exact tie of Q / s, a zero vector, one direction
    params, calls = ncases.plate_case(axis=0)
    state = define(sv, params, calls)
    centre = ncases.entry_of(state, (5, 5, 5))
    for table, want in (([[1, 0, 0, 0], [127, 0, 0, 0]], 0), ([[127, 0, 0, 9], [1, 0, 0, 0]], 0), ([[0, 0, 0, 0], [127, 0, 0, 0]], 1), ([[0, 1, 0, 0], [0, 0, 0, 5], [2, 0, 0, 0]], 2),
                        ([[5, 0, 0, 0]], 0), ([[0, 0, 0, 0]], -1), ([[0, 0, 0, 7], [0, 0, 0, 0]], -1)):
        got = _normals_agree(sv, state, np.array(table, np.int8))
        assert got["normal"][centre] == want, table
        if want < 0:
            assert got["fit"][centre].tolist() == [9, 0, 2 * C00, 0]  # no direction: lam1 = lam3 = 0
    one = _normals_agree(sv, state, np.array([[0, 3, 0, 0]], np.int8))  # K = 1 along the plate: lam1 = lam3 = C11, lam2 = T - 2 C11 = 0
    assert one["fit"][centre].tolist() == [9, C00, 0, C00] and one["normal"][centre] == -1


def test_thresholds(sv):
    params, calls = ncases.flat_threshold_case()
    state = define(sv, params, calls)
    centre = ncases.entry_of(state, (5, 5, 5))
    fit = _normals_agree(sv, state, AXES)["fit"][centre].tolist()
    assert fit == [5, 655360, 655360, 40960] and 256 * fit[3] == 16 * fit[2]
    for flat, want in ((16, 1), (15, -1), (17, 1), (0, -1), (256, 1)):
        assert _normals_agree(sv, state, AXES, flat=flat)["normal"][centre] == want, flat
    params, calls = ncases.wide_threshold_case()
    state = define(sv, params, calls)
    centre = ncases.entry_of(state, (5, 5, 5))
    fit = _normals_agree(sv, state, AXES)["fit"][centre].tolist()
    assert fit == [5, 1024000, 784000, 40960] and 256 * fit[2] == 196 * fit[1]
    for wide, want in ((196, 2), (197, -1), (195, 2), (0, 2), (256, -1)):
        assert _normals_agree(sv, state, AXES, wide=wide)["normal"][centre] == want, wide
    assert _normals_agree(sv, state, AXES, min_nb=6)["normal"][centre] == -1 and _normals_agree(sv, state, AXES, flat=13)["normal"][centre] == -1  # 256 * 40960 > 13 * 784000


def test_normals_against_the_model(sv):
    tables = (sv.voxel_normal_dirs(3), AXES, sv.voxel_normal_dirs(2, 5))
    given = members = 0
    for seed in range(30):
        params, calls = cases.random_case(seed)
        state = define(sv, params, calls)
        for filters in ncases.FILTERS:
            got = _normals_agree(sv, state, tables[seed % 3], min_nb=3 + seed % 4, **filters)
            given, members = given + int(got["counts"][2]), members + int(got["counts"][0])
    print("members %d, normals %d" % (members, given))
    assert members > 1000 and given > 100  # the cases reach the verdict both ways
    params, calls, _ = acases.edge_case()  # faces and corners of the box
    got = _normals_agree(sv, define(sv, params, calls), tables[0], min_nb=3)
    assert got["counts"][0] > 8
    params, calls, _ = acases.long_case()  # 2^20 cells on an axis: cell 2^20 is no cell
    got = _normals_agree(sv, define(sv, params, calls), tables[0], min_nb=3)
    assert got["fit"][:, 0].tolist() == [1, 1]  # neither is the other's neighbour
    params, calls, carve, _ = acases.tombstone_case()
    state = define(sv, params, calls)
    sv.voxel_map_carve(state, **carve, apply=True)
    for kw in (dict(min_n=1), dict(min_n=0), dict(min_n=-3, min_rows=-3, since=-2 ** 31)):
        got = _normals_agree(sv, state, tables[0], min_nb=3, **kw)
        assert got["counts"][0] == 1 and got["fit"].tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]]  # a tombstone is neither a member nor a neighbour
    over = define(sv, dict(BOX16, capacity=2), [cases.one_frame(cases.cell_points(cases.distinct_cells(3)))])
    got = _normals_agree(sv, over, tables[0])
    assert over["overflowed"] and (got["normal"] == -1).all() and not got["fit"].any() and not got["counts"].any()


HAND_DIRS = np.array([[2, 1, -2, 0], [3, -4, 12, 0]], np.int8)
HAND_NORMAL = np.array([1, -1, 0], np.int32)  # a, c, b in ascending key: a lies on direction 1, b on direction 0, c has none
HAND_ORIGIN = np.array([[100, 200, -50]], np.int32)


def _hand_words():
    """The 32 words of voxel_align_cases.hand_frame on the hand map: (weight, l = (p - o) >> 4, nu, b) of rows 0, 1 and 5."""
    pairs = [(1, (17, 19, 11), (3, -4, 12), 0), (3, (33, 19, 11), (3, -4, 12), 3 * -256), (2, (13, 27, 35), (2, 1, -2), 2 * 64 - 64)]
    rows = []
    for w, l, nu, b in pairs:
        a = [l[1] * nu[2] - l[2] * nu[1], l[2] * nu[0] - l[0] * nu[2], l[0] * nu[1] - l[1] * nu[0]] + list(nu)
        rows.append((w, a, b))
    assert [r[1][:3] for r in rows] == [[272, -171, -125], [272, -363, -189], [-89, 96, -41]]  # by hand
    want = [4, 3, 3, 6, 3 * 768 ** 2 + 2 * 64 ** 2] + [sum(w * a[i] * b for w, a, b in rows) for i in range(6)]
    want += [sum(w * a[i] * a[j] for w, a, _ in rows) for i in range(6) for j in range(i, 6)]
    assert want[4] == 1777664 and want[5] == 3 * 272 * -768 + 2 * -89 * 64 == -638080 and want[11] == 272 ** 2 + 3 * 272 ** 2 + 2 * 89 ** 2 == 311778
    assert want[31] == 144 + 3 * 144 + 2 * 4 and len(want) == 32
    return want


def test_plane_hand_case(sv):
    state = define(sv, HAND, acases.hand_calls())
    a, b, c = key_of((1, 2, 0)), key_of((1, 2, 1)), key_of((3, 2, 0))
    assert np.sort(state["key"]).tolist() == [a, c, b]
    before = {k: np.copy(v) for k, v in state.items() if isinstance(v, np.ndarray)}
    frame = acases.hand_frame()
    got = _planes_agree(sv, state, frame, IDENTITY[None], HAND_ORIGIN, HAND_NORMAL, HAND_DIRS)
    assert got["sums"].tolist() == [_hand_words()] and got["sums"].dtype == np.int64 and got["sums"].shape == (1, 32)
    assert got["pair_key"].tolist() == [[a, a, a, -1, -1, b]] and got["pair_normal"].tolist() == [[1, 1, 1, -1, -1, 0]] and got["pair_normal"].dtype == np.int32
    half = _planes_agree(sv, state, frame, IDENTITY[None], HAND_ORIGIN, HAND_NORMAL, HAND_DIRS, max_dist=0.5)  # rows 0 and 5 pair
    assert half["sums"][0, :5].tolist() == [4, 2, 2, 3, 2 * 64 ** 2] and same(half, got, PLANE_FIELDS[1:])
    none = _planes_agree(sv, state, frame, IDENTITY[None], HAND_ORIGIN, np.array([-1, 0, 2], np.int32), HAND_DIRS)  # a has none, b's word is no direction
    assert none["sums"][0].tolist() == [4, 3, 0] + [0] * 29 and none["pair_normal"].tolist() == [[-1] * 6]
    assert all(np.array_equal(state[k], v) for k, v in before.items())  # the map is not changed
    assert len(sv.VOXEL_PLANE_SUMS) == 32 and sv.VOXEL_PLANE_SUMS[11] == "A00" and sv.VOXEL_PLANE_SUMS[31] == "A55"


def test_plane_sums_against_the_model(sv):
    kinds, planes = set(), 0
    for seed in range(30):
        params, calls, frame, variants, origin, max_dist, filters = acases.random_align(seed)
        state = define(sv, params, calls)
        dirs = (sv.voxel_normal_dirs(3), AXES, sv.voxel_normal_dirs(2, 5))[seed % 3]
        normal = ncases.scrambled(sv.voxel_map_normals(state, dirs, min_nb=3, **filters)["normal"], len(dirs), seed)
        for v, poses in enumerate(variants):
            got = _planes_agree(sv, state, frame, poses, origin, normal, dirs, max_dist=max_dist, **filters)
            assert (got["sums"][1] == 0).all() and (got["pair_normal"][1] == -1).all()  # a count of 0 or -1
            assert v < 3 or (not got["sums"].any() and (got["pair_normal"] == -1).all())  # the pose that is not finite keeps nothing
            assert (got["sums"][:, 2] <= got["sums"][:, 1]).all() and (got["sums"][:, 3] >= got["sums"][:, 2]).all() and (got["sums"][:, 4] >= 0).all()
            planes += int(got["sums"][:, 2].sum())
        kinds.add((str(frame[0].dtype), frame[1] is None))
    assert len(kinds) == 4 and planes > 300


def _heavy_case(sv):
    rng = np.random.default_rng(9)
    fill = [cases.one_frame(rng.uniform(0.0, 16.0, (600, 3)))]
    xyz = rng.uniform(0.5, 15.5, (1, 3, 3))
    frame = (xyz, np.array([[2 ** 20 - 1, 2 ** 20 - 3, 2 ** 19 + 7]], np.int32), np.array([3], np.int32))
    origin = np.array([[-2 ** 20, 2 ** 20 - 7, -2 ** 20 + 3]], np.int32)  # |l| about 2^16, |a| about 2^24: w a^2 about 2^68 a row - the sums wrap
    near = np.array([[-2 ** 13, 2 ** 13 - 7, -2 ** 13 + 3]], np.int32)  # |l| about 2^9, |a| about 2^17: w a^2 about 2^54, inside the contract
    return fill, frame, origin, near


def test_plane_sums_of_64_bits(sv):
    fill, frame, origin, near = _heavy_case(sv)
    state = define(sv, BOX4K, fill)
    dirs = sv.voxel_normal_dirs()
    normal = np.arange(len(state["key"]), dtype=np.int32) % 513  # every voxel a plane pair's partner
    want = sv.voxel_map_align_plane_sums_brute(state, *frame, IDENTITY[None], near, normal, dirs, max_dist=2.0)
    assert want["sums"][0, 2] == 3 and 2 ** 50 < int(np.abs(want["sums"]).max()) < 2 ** 62  # far beyond 32 bits, and the definition far from wrapping
    assert same(sv.voxel_map_align_plane_sums(state, *frame, IDENTITY[None], near, normal, dirs, max_dist=2.0), want, PLANE_FIELDS)
    _planes_agree(sv, state, frame, IDENTITY[None], origin, normal, dirs, max_dist=2.0)  # beyond the contract both wrap alike: two's complement


def _own_pose_case(dtype):
    rng = np.random.default_rng(8)
    pts = cases.distinct_cells(200) + rng.uniform(0.01, 0.6, (200, 3))  # at most one row per cell, under the pose as well
    pts[7], pts[50] = np.nan, (20.0, 1.0, 1.0)
    return cases.one_frame(pts, None, None, shifted((0.3, 0.2, 0.1)), dtype)


def test_plane_own_pose(sv):
    for dtype in (np.float64, np.float32):
        call = _own_pose_case(dtype)
        state = define(sv, BOX16, [call])
        nr = sv.voxel_map_normals(state, sv.voxel_normal_dirs())
        kept = 200 - state["dropped"]
        origin = sv.voxel_align_origin(state["params"], call[4])
        got = _planes_agree(sv, state, (call[0], None, call[3]), call[4], origin, nr["normal"], nr["dirs"])
        planes = int(got["sums"][0, 2])
        assert planes == nr["counts"][2] > 50 and got["sums"][0, :5].tolist() == [kept, kept, planes, planes, 0] and not got["sums"][0, 5:11].any()  # E = 0, g = 0
        new, ok, step = sv.voxel_align_solve_plane(got["sums"], call[4], origin, state["params"])
        assert ok.tolist() == [True] and new.shape == (1, 12) and new.dtype == np.float64 and np.abs(new - call[4]).max() < 1e-12 and not step.any()


def test_accuracy_against_an_eigen_solver(sv):
    """On the scene of DESIGN.md 4r: the angle between the chosen direction and numpy's flattest eigenvector of the same covariance."""
    state = define(sv, mcases.SCENE_BOX, [acases.scene_case()[0]])
    d = sv.voxel_normal_dirs()
    got = sv.voxel_map_normals(state, d)
    assert got["counts"].tolist() == [978, 533, 491, 0]
    live, C = ncases.covariances(state)
    assert len(live) == 978
    vec = sv.voxel_normal_vectors(d, got["normal"])
    has = got["normal"] >= 0
    flattest = np.linalg.eigh(C)[1][:, :, 0]
    angle = np.degrees(np.arccos(np.clip(np.abs((vec * flattest).sum(1)), 0.0, 1.0)))[has]
    radius = ncases.covering_radius(d)
    print("angle to eigh's flattest eigenvector: median %.2f, largest %.2f degrees; the table's covering radius, sampled: %.2f" % (np.median(angle), angle.max(), radius))
    assert 4.0 < radius < 5.5 and np.median(angle) < radius


def test_convergence(sv):
    call, frame, truth = ncases.street()
    state = define(sv, ncases.STREET_BOX, [call])
    assert not state["overflowed"] and 6000 < len(state["key"]) < 9000
    nr = sv.voxel_map_normals(state, sv.voxel_normal_dirs())
    assert nr["counts"][2] > 0.9 * nr["counts"][0]
    start = ncases.street_start(truth)
    rot0, tr0 = acases.pose_error(start, truth)
    assert 0.499 < rot0 < 0.501 and 0.152 < tr0 < 0.154
    fr = (frame[None], None, np.array([len(frame)], np.int32))
    plane = sv.voxel_map_align(state, *fr, start[None], iterations=3, method="plane", normals=nr, eps=(0.0, 0.0))
    point = sv.voxel_map_align(state, *fr, start[None], iterations=10, eps=(0.0, 0.0))
    rot, tr = acases.pose_error(plane["poses"][0], truth)
    rot_p, tr_p = acases.pose_error(point["poses"][0], truth)
    print("street, from %.3f deg and %.4f m: plane after 3 rounds %.4f deg, %.4f m; point after 10 rounds %.4f deg, %.4f m" % (rot0, tr0, rot, tr, rot_p, tr_p))
    assert plane["rounds"] == 3 and point["rounds"] == 10 and plane["ok"].tolist() == [True]
    assert rot < 0.1 * rot0 and tr < 0.1 * tr0  # condition 1
    assert tr < 0.25 * tr_p                     # condition 2
    assert plane["sums"].shape == (1, 32) and plane["pairs"].shape == (3, 1) and plane["pairs"][-1, 0] == plane["sums"][0, 2] > 5000 and plane["rms"][-1, 0] < plane["rms"][0, 0]
    assert int(np.abs(plane["sums"]).max()) < 2 ** 50
    fitted = sv.voxel_map_align(state, *fr, start[None], iterations=3, method="plane", eps=(0.0, 0.0))  # normals=None fits them with the defaults
    assert np.array_equal(fitted["poses"], plane["poses"])
    ground = frame[np.abs(frame[:, 2] + truth[11]) < 0.05]  # the rows of the ground plane alone
    assert len(ground) > 2000
    res = sv.voxel_map_align(state, ground[None], None, np.array([len(ground)], np.int32), start[None], iterations=2, method="plane", normals=nr)
    R0, R = start[:9].reshape(3, 3), res["poses"][0, :9].reshape(3, 3)
    print("ground rows only, 2 rounds: R20, R21 %s -> %s, z %.4f -> %.4f" % (R0[2, :2], R[2, :2], start[11] - truth[11], res["poses"][0, 11] - truth[11]))
    assert res["ok"].tolist() == [True] and (np.abs(R[2, :2]) < 0.1 * np.abs(R0[2, :2])).all() and abs(res["poses"][0, 11] - truth[11]) < 0.1 * abs(start[11] - truth[11])
    # the scene of DESIGN.md 4r: both methods end at the same place, plane in fewer rounds; dof 4 leaves roll and pitch alone
    state = define(sv, mcases.SCENE_BOX, [acases.scene_case()[0]])
    frame4, truth4 = acases.scene_case()[1], acases.scene_truth(sv)
    start4 = acases.scene_start(sv, *acases.SCENE_STARTS["all"])
    plane = sv.voxel_map_align(state, *frame4, start4[None], iterations=15, method="plane")
    point = sv.voxel_map_align(state, *frame4, start4[None], iterations=15)
    rot, tr = acases.pose_error(plane["poses"][0], truth4)
    print("scene: plane %.4f deg, %.4f m in %d rounds; point in %d rounds" % (rot, tr, plane["rounds"], point["rounds"]))
    assert rot < 0.27 and tr < 0.0141 and plane["rounds"] < point["rounds"]  # a tenth of the start's 2.69 degrees and 0.141 m
    yaw_only = sv.voxel_map_align(state, *frame4, start4[None], iterations=5, method="plane", dof=4)
    assert np.array_equal(yaw_only["poses"][0, 6:9], start4[6:9]) and yaw_only["ok"].tolist() == [True]
    cpu = util.pkg("rig").VoxelMap(device="cpu", **mcases.SCENE_BOX)  # rig.VoxelMap on CPU tensors runs the definition
    cpu.update(*acases.scene_case()[0])
    poses, result = cpu.align(*frame4, start4[None], iterations=15, method="plane")
    assert np.array_equal(poses, plane["poses"]) and result.rounds == plane["rounds"] and np.array_equal(result.sums.numpy(), plane["sums"])
    assert cpu._normals_fresh and cpu.normals()["counts"].tolist() == [978, 533, 491, 0]
    cpu.update(*acases.scene_case()[0])
    assert not cpu._normals_fresh


def test_refusals(sv):
    state = define(sv, BOX16, [cases.one_frame(cases.cell_points(cases.distinct_cells(40)))])
    d = sv.voxel_normal_dirs(2)
    for kw in (dict(min_nb=2), dict(min_nb=28), dict(min_nb=5.5), dict(flat=-1), dict(flat=257), dict(wide=-1), dict(wide=257), dict(wide=True), dict(dirs=d.astype(np.int16)),
               dict(dirs=d[:, :3]), dict(dirs=d[:0]), dict(dirs=np.zeros((4097, 4), np.int8)), dict(dirs=d[0])):
        for f in (sv.voxel_map_normals, sv.voxel_map_normals_brute):
            with pytest.raises(ValueError):
                f(state, **dict(dict(dirs=d), **kw))
    assert sv.voxel_map_normals(state, np.zeros((4096, 4), np.int8))["counts"][[0, 2]].tolist() == [40, 0]  # the largest table, of zero vectors
    xyz, counts = cases.cell_points(cases.distinct_cells(40), 0.25)[None], np.array([40], np.int32)
    normal = np.zeros(40, np.int32)
    good = dict(xyz=xyz, n=None, counts=counts, poses=IDENTITY[None], origin=ZERO, normal=normal, dirs=d)
    assert sv.voxel_map_align_plane_sums(state, **good)["sums"][0, :4].tolist() == [40, 40, 40, 40]
    for kw in (dict(max_dist=-0.5), dict(max_dist=np.nan), dict(poses=np.zeros((2, 12))), dict(origin=np.zeros((1, 3))), dict(origin=np.array([[2 ** 30 + 1, 0, 0]])),
               dict(xyz=np.zeros((1, 40, 2))), dict(counts=np.zeros(2, np.int32)), dict(n=np.zeros((1, 3), np.int32)), dict(normal=np.zeros(39, np.int32)),
               dict(normal=np.zeros(40, np.int64)), dict(normal=np.zeros((40, 1), np.int32)), dict(dirs=d[:, :3]), dict(dirs=np.zeros((0, 4), np.int8))):
        for f in (sv.voxel_map_align_plane_sums, sv.voxel_map_align_plane_sums_brute):
            with pytest.raises(ValueError):
                f(state, **dict(good, **kw))
    loop = dict(xyz=xyz, n=None, counts=counts, poses=IDENTITY[None])
    for kw in (dict(method="planes"), dict(method=None), dict(method="point", normals=sv.voxel_map_normals(state, d)), dict(method="plane", dof=5), dict(method="plane", eps=(1e-5,)),
               dict(method="plane", iterations=-1), dict(method="plane", max_dist=-1.0)):
        with pytest.raises(ValueError):
            sv.voxel_map_align(state, **dict(loop, **kw))
    sums = sv.voxel_map_align_plane_sums(state, **good)["sums"]
    for args in ((sums, IDENTITY[None], ZERO, state["params"], 5), (sums[:, :19], IDENTITY[None], ZERO, state["params"]), (sums, IDENTITY[None], np.zeros((1, 2), np.int32), state["params"]),
                 (sums, IDENTITY[None], ZERO, state["params"], 6, 6, -1.0), (sums, IDENTITY[None], ZERO, state["params"], 6, 1.5)):
        with pytest.raises(ValueError):
            sv.voxel_align_solve_plane(*args)
    start = shifted((0.1, 0.05, -0.1))
    kept, ok, step = sv.voxel_align_solve_plane(sums, start[None], ZERO, state["params"], min_pairs=41)  # 40 planes: too few
    assert np.array_equal(kept[0], start) and ok.tolist() == [False] and step.tolist() == [[0.0, 0.0]]
    res = sv.voxel_map_align(state, xyz, None, counts, start[None], method="plane", min_pairs=41)
    assert np.array_equal(res["poses"][0], start) and res["ok"].tolist() == [False] and res["rounds"] == 1 and res["sums"].shape == (1, 32)
    empty = sv.voxel_map_align(state, np.zeros((0, 4, 3)), None, np.zeros(0, np.int32), np.zeros((0, 12)), method="plane")
    assert empty["poses"].shape == (0, 12) and empty["sums"].shape == (0, 32)
    assert sv.cli_voxel_align_spec("3") == (3, 1.0, 6, "point") and sv.cli_voxel_align_spec("3,1.5,4,plane") == (3, 1.5, 4, "plane")
    for bad in ("3,1,6,planes", "3,1,6,plane,1", "3,1,6,"):
        with pytest.raises(ValueError):
            sv.cli_voxel_align_spec(bad)
    # what every existing call returns is what it returned: the default solver and eps are the point method's
    a = sv.voxel_map_align(state, xyz, None, counts, start[None], iterations=4)
    b = sv.voxel_map_align(state, xyz, None, counts, start[None], iterations=4, eps=(1e-5, 1.0 / 256), method="point")
    assert all(np.array_equal(a[k], b[k]) for k in ("poses", "ok", "sums", "pairs", "rms")) and a["sums"].shape == (1, 19)


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z_]*voxel_(?:normals|plane_align)[a-z_]*)\s*\(", src))
    assert declared == {"sv_voxel_normals_device", "sv_voxel_plane_align_workspace", "sv_voxel_plane_align_device", "sv_debug_voxel_normals"}
    assert text.index("/* ---- (X)") < text.index("/* ---- (Y)") < text.index("/* ---- (A)") and " *  (Y) " in text
    assert set(util.pkg("engine").STAGE_SIGNATURES["voxel_normals"]) == declared
    build = util.pkg("build")
    assert "voxel_normal_kernels.hip" in build.SOURCES and "voxel_normals.cpp" in build.SOURCES and "voxel_normal_kernels.h" in build.HEADERS
    assert all(n in sv.__doc__ for n in ("voxel_map_normals", "voxel_map_align_plane_sums", "voxel_align_solve_plane")) and "(Y)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_normal_kernels.hip")).read()
    assert "asm" not in source and source.count("atomicAdd(") == 1  # the counts' flush
    squeezed = cases.squeeze(source)
    assert '#include "voxel_map_table.h"' in source and all(cases.squeeze(t) not in squeezed for t in cases.TABLE_TEXTS)  # the map's rules are the table's
    assert all(source.count(call) == 1 for call in ("vmap_cell(", "vmap_offset(", "vmap_probe_goes_on(", "vmap_next_slot(", "vmap_slot_of("))  # one probe, one row's way
    assert "wave_sum(" in source and "__shfl" not in source and "h + 1" not in source
    kernels = open(os.path.join(build.CSRC, "voxel_normal_kernels.h")).read()
    assert re.search(r"VPLANE_WORDS = 32,", kernels) and re.search(r"VNORMAL_DIRS_MAX = 4096,", kernels) and re.search(r"VPLANE_LEVER_SHIFT = 4,", kernels)
    assert sv.VOXEL_PLANE_LEVER_SHIFT == 4 and sv.VOXEL_NORMAL_DIRS_MAX == 4096


# ---------------------------------------------------------------------------------------------------------------- GPU

def _engine_map(eng, sv, params, calls):
    words = sv.voxel_map_params(**params)
    buf, seq = eng.voxel_map_new(words), 0
    for call in calls:
        eng.voxel_map_insert(buf, words, *[None if a is None else _cuda(a) for a in call[:4]], call[4], seq0=seq)
        seq += call[0].shape[0]
    return buf, words


def _gpu_normals(eng, buf, words, dirs, want_fit=True, **kw):
    res = eng.voxel_map_normals(buf, words, dirs, want_fit=want_fit, **kw)
    key, normal, fit = eng.voxel_normal_labels(res)
    out = {"key": key.cpu().numpy(), "normal": normal.cpu().numpy(), "counts": res.counts.cpu().numpy(), "fit": None if fit is None else fit.cpu().numpy()}
    assert (res.normal.cpu().numpy()[res.keys.cpu().numpy() == -1] == -1).all() and str(res.normal.dtype) == "torch.int32"  # an empty slot has no normal
    return out, res


def _normals_on_device(eng, sv, buf, words, state, dirs, **kw):
    """The device's normals, with and without fit and with the pruning on and off, against the definition's - through the keys."""
    want = sv.voxel_map_normals(state, dirs, **kw)
    try:
        for prune in (True, False):
            assert eng.debug_voxel_normals(0, True, prune) == 0
            got, _ = _gpu_normals(eng, buf, words, dirs, **kw)
            assert same(got, want, NORMAL_FIELDS), (kw, prune, np.flatnonzero(got["normal"] != want["normal"])[:8], got["counts"], want["counts"])
            bare, res = _gpu_normals(eng, buf, words, dirs, want_fit=False, **kw)
            assert same(bare, want, ("normal", "counts", "key")) and res.fit is None, (kw, prune)
    finally:
        eng.debug_voxel_normals(0, True, True)
    return want


@pytest.mark.gpu
def test_the_normal_cases_on_the_device(sv, eng):
    d = sv.voxel_normal_dirs()
    for params, calls in (ncases.plate_case(), ncases.plate_case(axis=0), ncases.column_case(), (BOX16, ncases.one_voxel_each([ncases.at_sub((5, 5, 5), (1, 2, 3))]))):
        buf, words = _engine_map(eng, sv, params, calls)
        state = define(sv, params, calls)
        for table in (d, AXES, np.array([[1, 0, 0, 0], [127, 0, 0, 0]], np.int8), np.array([[0, 0, 0, 0], [127, 0, 0, 0]], np.int8), np.array([[0, 0, 0, 0]], np.int8),
                      np.array([[0, 3, 0, 0]], np.int8)):
            for min_nb in (3, 5):
                _normals_on_device(eng, sv, buf, words, state, table, min_nb=min_nb)
    for case, values in ((ncases.flat_threshold_case(), [dict(flat=v) for v in (15, 16, 17, 0, 256)]), (ncases.wide_threshold_case(), [dict(wide=v) for v in (195, 196, 197, 0, 256)])):
        buf, words = _engine_map(eng, sv, *case)
        state = define(sv, *case)
        seen = [int(_normals_on_device(eng, sv, buf, words, state, AXES, **kw)["counts"][2]) for kw in values]
        assert seen == ([0, 1, 1, 0, 1] if "flat" in values[0] else [1, 1, 0, 1, 0])  # exactly at the threshold, and one unit to either side
    tables = (sv.voxel_normal_dirs(3), AXES, sv.voxel_normal_dirs(2, 5))
    given = 0
    for seed in range(30):
        params, calls = cases.random_case(seed)
        buf, words = _engine_map(eng, sv, params, calls)
        state = define(sv, params, calls)
        given += int(_normals_on_device(eng, sv, buf, words, state, tables[seed % 3], min_nb=3 + seed % 4, **ncases.FILTERS[seed % 3])["counts"][2])
    assert given > 30
    for params, calls, _ in (acases.edge_case(), acases.long_case()):
        buf, words = _engine_map(eng, sv, params, calls)
        _normals_on_device(eng, sv, buf, words, define(sv, params, calls), tables[0], min_nb=3)
    params, calls, carve, _ = acases.tombstone_case()
    buf, words = _engine_map(eng, sv, params, calls)
    state = define(sv, params, calls)
    sv.voxel_map_carve(state, **carve, apply=True)
    eng.voxel_map_carve(buf, words, _cuda(carve["xyz"]), None, _cuda(carve["counts"]), carve["poses"], origin=carve["origin"], seq0=1, apply=True)
    for kw in (dict(min_n=1), dict(min_n=0), dict(min_n=-3, min_rows=-3, since=-2 ** 31)):
        assert _normals_on_device(eng, sv, buf, words, state, tables[0], min_nb=3, **kw)["counts"][0] == 1
    over = dict(BOX16, capacity=2)
    calls = [cases.one_frame(cases.cell_points(cases.distinct_cells(3)))]
    buf, words = _engine_map(eng, sv, over, calls)
    assert not _normals_on_device(eng, sv, buf, words, define(sv, over, calls), tables[0])["counts"].any()


@pytest.mark.gpu
def test_table_sizes_and_workgroups(sv, eng):
    rng = np.random.default_rng(21)
    fill = [cases.one_frame(rng.uniform(0.0, 16.0, (3000, 3)), None, rng.integers(1, 9, 3000), dtype=np.float32)]
    buf, words = _engine_map(eng, sv, BOX4K, fill)  # 8192 slots: 32 workgroups
    state = define(sv, BOX4K, fill)
    assert not state["overflowed"] and len(state["key"]) > 2000
    big = rng.integers(-127, 128, (4096, 4)).astype(np.int8)
    big[[0, 1023, 1024, 2500]] = 0  # zero vectors at a tile's edges
    for K in (1, 63, 64, 65, 513, 1024, 1025, 4096):  # 1024 directions are staged at a time
        table = sv.voxel_normal_dirs() if K == 513 else big[-K:].copy()
        want = _normals_on_device(eng, sv, buf, words, state, table, min_nb=5 + K % 3, flat=256, wide=0)  # a random cloud: blobs, which these let through
        assert want["counts"][0] == len(state["key"]) and (K < 63 or want["counts"][2] > 50)


@pytest.mark.gpu
def test_probe_chains(sv, eng):
    import torch
    block = cases.distinct_cells(8 * 8 * 7, 8) + np.array([20, 20, 20])  # a dense block, every voxel with all its neighbours
    for slot in (500, 1023):  # colliding keys; from the last slot the probes wrap to the table's start
        cells = cases.colliding_cells(sv.voxel_map_slot_of, slot, 8)
        near = np.clip(cells + np.array([1, 0, 0]), 0, 63)  # a neighbour for each of them
        every = np.unique(np.concatenate([cells, near, block]), axis=0)
        calls = [cases.one_frame(cases.cell_points(cells), dtype=np.float32), cases.one_frame(every + np.random.default_rng(slot).uniform(0.1, 0.9, every.shape), dtype=np.float32)]
        buf, words = _engine_map(eng, sv, PROBE_BOX, calls)
        state = define(sv, PROBE_BOX, calls)
        assert not state["overflowed"] and 460 < len(state["key"]) <= 512  # a table of 1024 slots as full as its capacity allows
        before = buf.clone()
        want = _normals_on_device(eng, sv, buf, words, state, sv.voxel_normal_dirs(4), min_nb=3)
        assert want["counts"][1] > 440
        torch.cuda.synchronize()
        assert torch.equal(buf, before)  # the map is only read


def _gpu_planes(eng, buf, words, frame, poses, origin, normals, want_rows=True, **kw):
    xyz, n, counts = frame
    res = eng.voxel_map_align_plane_sums(buf, words, _cuda(xyz), None if n is None else _cuda(n), _cuda(counts), poses, origin, normals, want_rows=want_rows, **kw)
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in PLANE_FIELDS}


def _slot_normals(eng, buf, words, normal_by_key, dirs):
    """A per-slot normal array from one per entry in ascending key -> (int32 tensor [slots], the table on the device)."""
    import torch
    slots = util.pkg("stereo_vision.sv").voxel_map_slots(words["capacity"])
    keys = buf[4:].as_strided((slots,), (11,)).cpu().numpy()
    at = np.flatnonzero(keys != -1)
    out = np.full(slots, -1, np.int32)
    out[at[np.argsort(keys[at], kind="stable")]] = normal_by_key
    return torch.from_numpy(out).cuda(), eng.voxel_normal_table(dirs, buf.device)


def _planes_on_device(eng, sv, buf, words, state, frame, poses, origin, normal, dirs, **kw):
    """The device's dict, with and without the per-row outputs, against the definition's."""
    want = sv.voxel_map_align_plane_sums(state, *frame, poses, origin, normal, dirs, **kw)
    normals = _slot_normals(eng, buf, words, normal, dirs)
    got = _gpu_planes(eng, buf, words, frame, poses, origin, normals, **kw)
    assert same(got, want, PLANE_FIELDS), (kw, np.flatnonzero(got["sums"] != want["sums"]), np.flatnonzero(got["pair_normal"] != want["pair_normal"])[:8])
    bare = _gpu_planes(eng, buf, words, frame, poses, origin, normals, want_rows=False, **kw)
    assert same(bare, want, PLANE_FIELDS[:1]) and bare["pair_key"] is None and bare["pair_normal"] is None, kw
    return got


@pytest.mark.gpu
def test_the_plane_cases_on_the_device(sv, eng):
    buf, words = _engine_map(eng, sv, HAND, acases.hand_calls())
    got = _planes_on_device(eng, sv, buf, words, define(sv, HAND, acases.hand_calls()), acases.hand_frame(), IDENTITY[None], HAND_ORIGIN, HAND_NORMAL, HAND_DIRS)
    assert got["sums"].tolist() == [_hand_words()]
    kinds, planes = set(), 0
    for seed in range(30):  # B = 3: a frame with its rows, one with a count of 0 or -1, one with a count above cap; four poses, one not finite
        params, calls, frame, variants, origin, max_dist, filters = acases.random_align(seed)
        buf, words = _engine_map(eng, sv, params, calls)
        state = define(sv, params, calls)
        dirs = (sv.voxel_normal_dirs(3), AXES, sv.voxel_normal_dirs(2, 5))[seed % 3]
        normal = ncases.scrambled(sv.voxel_map_normals(state, dirs, min_nb=3, **filters)["normal"], len(dirs), seed)
        for poses in variants:
            planes += int(_planes_on_device(eng, sv, buf, words, state, frame, poses, origin, normal, dirs, max_dist=max_dist, **filters)["sums"][:, 2].sum())
        kinds.add((str(frame[0].dtype), frame[1] is None))
    assert len(kinds) == 4 and planes > 300
    for dtype in (np.float64, np.float32):
        call = _own_pose_case(dtype)
        buf, words = _engine_map(eng, sv, BOX16, [call])
        state = define(sv, BOX16, [call])
        nr = sv.voxel_map_normals(state, sv.voxel_normal_dirs())
        got = _planes_on_device(eng, sv, buf, words, state, (call[0], None, call[3]), call[4], sv.voxel_align_origin(words, call[4]), nr["normal"], nr["dirs"])
        assert got["sums"][0, 2] > 50 and not got["sums"][0, 4:11].any()
        res = eng.voxel_map_align_plane_sums(buf, words, _cuda(call[0]), None, _cuda(call[3]), call[4], sv.voxel_align_origin(words, call[4]), eng.voxel_map_normals(buf, words))
        assert np.array_equal(res.sums.cpu().numpy(), got["sums"])  # the device's own normals, handed on as they are
    fill, frame, origin, near = _heavy_case(sv)
    buf, words = _engine_map(eng, sv, BOX4K, fill)
    state = define(sv, BOX4K, fill)
    normal = np.arange(len(state["key"]), dtype=np.int32) % 513
    for o in (near, origin):
        got = _planes_on_device(eng, sv, buf, words, state, frame, IDENTITY[None], o, normal, sv.voxel_normal_dirs(), max_dist=2.0)
        assert same(got, sv.voxel_map_align_plane_sums_brute(state, *frame, IDENTITY[None], o, normal, sv.voxel_normal_dirs(), max_dist=2.0), PLANE_FIELDS)
    over = dict(BOX16, capacity=2)
    calls = [cases.one_frame(cases.cell_points(cases.distinct_cells(3)))]
    buf, words = _engine_map(eng, sv, over, calls)
    state = define(sv, over, calls)
    got = _planes_on_device(eng, sv, buf, words, state, (calls[0][0], None, calls[0][3]), IDENTITY[None], ZERO, np.zeros(len(state["key"]), np.int32), AXES)
    assert not got["sums"].any() and (got["pair_key"] == -1).all() and (got["pair_normal"] == -1).all()


@pytest.mark.gpu
def test_row_counts(sv, eng):
    rng = np.random.default_rng(21)
    fill = [cases.one_frame(rng.uniform(0.0, 16.0, (3000, 3)), None, rng.integers(1, 9, 3000), dtype=np.float32)]
    buf, words = _engine_map(eng, sv, BOX4K, fill)
    state = define(sv, BOX4K, fill)
    dirs = sv.voxel_normal_dirs()
    normal = sv.voxel_map_normals(state, dirs, flat=256, wide=0)["normal"]  # a random cloud: blobs, which these let through
    assert (normal >= 0).sum() > 500
    text = open(os.path.join(util.pkg("build").CSRC, "voxel_normal_kernels.h")).read()
    chunk = int(re.search(r"\bVPLANE_THREADS = (\d+),", text).group(1))
    assert "VPLANE_CHUNK = VPLANE_THREADS," in text and chunk == 256

    def frame_of(rows, B=1):
        cap = rows + 5 + ((rows + 5) % 64 == 0)  # never a multiple of 64
        xyz = rng.uniform(-1.0, 17.0, (B, cap, 3)).astype(np.float32 if rows % 2 else np.float64)
        return (xyz, rng.integers(-1, 9, (B, cap)).astype(np.int32), np.full(B, rows, np.int32))

    pose = lambda: shifted(rng.uniform(-0.4, 0.4, 3))  # noqa: E731
    for rows in (0, 1, 63, 65, chunk - 1, chunk, chunk + 1):
        got = _planes_on_device(eng, sv, buf, words, state, frame_of(rows), pose()[None], rng.integers(-3000, 6000, (1, 3)).astype(np.int32), normal, dirs, max_dist=(1.0, 2.0)[rows % 2])
        assert got["sums"][0, 0] <= rows and (got["sums"][0, 2] > 0 or rows < 16) and (got["pair_normal"][0, rows:] == -1).all()
    frame = frame_of(2 * chunk + 1, B=3)  # three frames, one of them empty; under the hook a workgroup takes all three chunks of a frame
    frame[2][:] = (2 * chunk + 1, 0, chunk)
    poses, origin = np.stack([pose() for _ in range(3)]), rng.integers(-3000, 6000, (3, 3)).astype(np.int32)
    seen = []
    try:
        for max_chunks, skip in ((0, True), (1, True), (2, True), (0, False), (2, False)):
            assert eng.debug_voxel_normals(max_chunks, skip) == 0
            seen.append(_planes_on_device(eng, sv, buf, words, state, frame, poses, origin, normal, dirs))
        assert all(same(s, seen[0], PLANE_FIELDS) for s in seen) and seen[0]["sums"][0, 2] > 3 and not seen[0]["sums"][1].any()
        assert eng.debug_voxel_normals(-1) == SV_ERR_ARG and eng.debug_voxel_normals(513) == SV_ERR_ARG
    finally:
        eng.debug_voxel_normals(0, True, True)
    normals = _slot_normals(eng, buf, words, normal, dirs)
    none = _gpu_planes(eng, buf, words, (np.zeros((0, 40, 3), np.float32), None, np.zeros(0, np.int32)), np.zeros((0, 12)), np.zeros((0, 3), np.int32), normals)
    assert none["sums"].shape == (0, 32) and none["pair_normal"].shape == (0, 40)
    no_rows = _planes_on_device(eng, sv, buf, words, state, (np.zeros((2, 0, 3)), None, np.array([0, 5], np.int32)), np.stack([IDENTITY] * 2), np.zeros((2, 3), np.int32), normal, dirs)
    assert not no_rows["sums"].any() and no_rows["pair_key"].shape == (2, 0)  # cap 0: no score kernel, the sums written


@pytest.mark.gpu
def test_the_loop_on_the_device(sv, eng):
    rigmod = util.pkg("rig")
    truth = acases.scene_truth(sv)
    for dtype, dof in ((np.float64, 6), (np.float32, 6), (np.float64, 4)):
        call, (xyz, n, counts) = acases.scene_case(dtype)
        worlds = [rigmod.VoxelMap(device=d, **mcases.SCENE_BOX) for d in ("cuda", "cpu")]
        worlds[0].update(*[None if a is None else _cuda(a) for a in call[:4]], call[4])
        worlds[1].update(*call)
        start = acases.scene_start(sv, *acases.SCENE_STARTS["all"])[None]
        want = sv.voxel_map_align(worlds[1]._state, xyz, n, counts, start, iterations=15, dof=dof, method="plane")
        res = eng.voxel_map_align(worlds[0].buffer, worlds[0].params, _cuda(xyz), None, _cuda(counts), start, iterations=15, dof=dof, method="plane")
        assert isinstance(res, eng.VoxelPlaneResult) and res.sums.is_cuda and res.poses.dtype == np.float64
        for k in ("poses", "ok", "pairs", "rms"):
            assert np.array_equal(getattr(res, k), want[k]) and getattr(res, k).dtype == want[k].dtype, k  # equal, not close: the fit is shared and the sums are equal
        assert res.rounds == want["rounds"] and np.array_equal(res.sums.cpu().numpy(), want["sums"])
        (poses, got), (poses_cpu, got_cpu) = (w.align(x, None, c, p, iterations=15, dof=dof, method="plane") for w, x, c, p in
                                              ((worlds[0], _cuda(xyz), _cuda(counts), _cuda(start)), (worlds[1], xyz, counts, start)))
        assert np.array_equal(poses, poses_cpu) and np.array_equal(poses, want["poses"]) and got.rounds == got_cpu.rounds == want["rounds"]
        rot0, tr0 = acases.pose_error(start[0], truth)
        rot, tr = acases.pose_error(poses[0], truth)
        assert dof == 4 or (rot < rot0 / 10 and tr < tr0 / 10)
        assert worlds[0].stats() == {"claimed": 978, "dropped": 0, "overflowed": False} and worlds[0].seq == 1
    vm = worlds[0]
    worlds.append(rigmod.VoxelMap(device="cuda", **mcases.SCENE_BOX))  # another map, to merge
    kept = vm._normals[1]
    assert vm._normals_fresh and kept.counts.cpu().numpy().tolist() == [978, 533, 491, 0]
    again = vm.normals()
    assert again is kept and vm._normals_fresh  # written into the tensors the map keeps
    more = cases.one_frame(np.array([[3.1, 3.1, 1.1], [3.4, 3.1, 1.1], [3.1, 3.4, 1.1]]))  # three voxels more: the kept normals are stale
    vm.update(*[None if a is None else _cuda(a) for a in more[:4]], more[4])
    worlds[1].update(*more)
    assert not vm._normals_fresh and not worlds[1]._normals_fresh
    (poses, got), (poses_cpu, got_cpu) = (w.align(x, None, c, p, iterations=3, method="plane") for w, x, c, p in ((vm, _cuda(xyz), _cuda(counts), start), (worlds[1], xyz, counts, start)))
    assert vm._normals_fresh and vm._normals[1].counts.cpu().numpy().tolist() == worlds[1]._normals[1]["counts"].tolist() and vm._normals[1].counts[0].item() == 981  # fitted again: three voxels more
    assert np.array_equal(poses, poses_cpu) and np.array_equal(got.sums.cpu().numpy(), got_cpu.sums.numpy())
    for change in (lambda w: w.prune(), lambda w: w.despeckle(2), lambda w: w.resize(8192), lambda w: w.recenter(10.0, 8.0), lambda w: w.merge(worlds[2]),
                   lambda w: w.carve(_cuda(xyz), None, _cuda(counts), start, apply=True), lambda w: w.reset()):
        vm.normals()
        assert vm._normals_fresh
        change(vm)
        assert not vm._normals_fresh
    assert vm.normals(m=8, min_nb=4).dirs.shape[0] == 129
    for kw in (dict(method="planes"), dict(method="plane", normals=(1, 2)), dict(method="point", normals=kept), dict(method="plane", dof=5)):
        with pytest.raises(ValueError):
            eng.voxel_map_align(worlds[0].buffer, worlds[0].params, **dict(dict(xyz=_cuda(xyz), n=None, counts=_cuda(counts), poses=start), **kw))
    fresh = eng.voxel_map_normals(vm.buffer, vm.params)
    for kw in (dict(normals=(fresh.normal[:-1], fresh.dirs)), dict(normals=(fresh.normal.long(), fresh.dirs)), dict(normals=(fresh.normal, fresh.dirs[:, :3])),
               dict(normals=(fresh.normal.cpu(), fresh.dirs)), dict(origin=np.zeros((2, 3), np.int32)), dict(max_dist=np.nan)):
        with pytest.raises(ValueError):
            eng.voxel_map_align_plane_sums(vm.buffer, vm.params, **dict(dict(xyz=_cuda(xyz), n=None, counts=_cuda(counts), poses=start, origin=ZERO, normals=fresh), **kw))
    for kw in (dict(min_nb=2), dict(flat=257), dict(wide=-1), dict(dirs=np.zeros((0, 4), np.int8)), dict(dirs=fresh.dirs.cpu()), dict(min_n=0.5), dict(since=2 ** 31)):
        with pytest.raises(ValueError):
            eng.voxel_map_normals(vm.buffer, vm.params, **kw)


@pytest.mark.gpu
def test_the_c_entries_refuse(sv, eng):
    import ctypes
    import torch
    words = sv.voxel_map_params(**BOX16)
    buf, _ = _engine_map(eng, sv, BOX16, [cases.one_frame(cases.cell_points(cases.distinct_cells(40)), dtype=np.float32)])
    before = buf.clone()
    L = eng.voxel_normals_lib()
    spec, nbytes, st = eng.voxel_map_spec(words), buf.numel() * 8, torch.cuda.current_stream().cuda_stream
    dirs = eng.voxel_normal_table(sv.voxel_normal_dirs(2), buf.device)
    slots = 1024
    out = {k: torch.full(shape, 77, dtype=dt, device="cuda") for k, shape, dt in (("normal", (slots,), torch.int32), ("fit", (slots, 4), torch.int64), ("counts", (4,), torch.int64))}

    def spec_with(**kw):
        s = eng.voxel_map_spec(words)
        for k, v in kw.items():
            if k in ("lo", "hi", "reserved"):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return ctypes.byref(s)

    good = [buf.data_ptr(), nbytes, ctypes.byref(spec), dirs.data_ptr(), 9, 5, 64, 16, 1, 1, 0, out["normal"].data_ptr(), slots, out["fit"].data_ptr(), out["counts"].data_ptr(), st]
    bad = {0: [None, buf.data_ptr() + 8], 1: [nbytes - 8, 0], 2: [None, spec_with(size=0.0), spec_with(capacity=0), spec_with(reserved=(3, 1)), spec_with(hi=(1, 0.0))],
           3: [None, dirs.data_ptr() + 2], 4: [0, -1, 4097], 5: [2, 28], 6: [-1, 257], 7: [-1, 257], 11: [None, out["normal"].data_ptr() + 2, buf.data_ptr() + 64],
           12: [slots - 1, slots + 1, 2 * slots, 0], 13: [out["fit"].data_ptr() + 4, out["normal"].data_ptr()], 14: [None, out["counts"].data_ptr() + 4, out["fit"].data_ptr()]}
    for at, values in bad.items():
        for v in values:
            assert L.sv_voxel_normals_device(*(good[:at] + [v] + good[at + 1:])) == SV_ERR_ARG and b"sv_voxel_normals" in L.sv_last_error(None), (at, v)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and all((t == 77).all().item() for t in out.values())  # nothing was enqueued
    want = sv.voxel_map_normals(define(sv, BOX16, [cases.one_frame(cases.cell_points(cases.distinct_cells(40)), dtype=np.float32)]), sv.voxel_normal_dirs(2))
    assert L.sv_voxel_normals_device(*(good[:13] + [None] + good[14:])) == 0  # without fit
    torch.cuda.synchronize()
    assert out["counts"].tolist() == want["counts"].tolist() and want["counts"][2] > 10 and (out["fit"] == 77).all().item() and int((out["normal"] >= 0).sum()) == want["counts"][2]
    assert L.sv_voxel_normals_device(*good) == 0 and L.sv_voxel_normals_device(*(good[:4] + [1] + good[5:])) == 0  # and with it; a table of one direction
    torch.cuda.synchronize()
    assert int((out["fit"][:, 0] > 0).sum()) == 40 and torch.equal(buf, before)

    xyz, n, counts = _cuda(cases.cell_points(cases.distinct_cells(40)).astype(np.float32)[None]), _cuda(np.full((1, 40), 2, np.int32)), _cuda(np.array([40], np.int32))
    poses, origin = _cuda(IDENTITY[None]), _cuda(ZERO)
    normal = torch.zeros((slots,), dtype=torch.int32, device="cuda")
    need = ctypes.c_size_t(7)
    for cap, B in ((-1, 1), (40, -1), (40, 65536)):
        assert L.sv_voxel_plane_align_workspace(cap, B, ctypes.byref(need)) == SV_ERR_ARG and need.value == 7 and b"sv_voxel_plane_align" in L.sv_last_error(None)
    assert L.sv_voxel_plane_align_workspace(40, 1, None) == SV_ERR_ARG
    assert L.sv_voxel_plane_align_workspace(257, 3, ctypes.byref(need)) == 0 and need.value == 3 * 2 * 32 * 8
    assert L.sv_voxel_plane_align_workspace(2 ** 31 - 1, 2, ctypes.byref(need)) == 0 and need.value == 2 * 512 * 32 * 8
    assert L.sv_voxel_plane_align_workspace(40, 1, ctypes.byref(need)) == 0 and need.value == 32 * 8
    ws = torch.full((need.value // 8 + 2,), 77, dtype=torch.int64, device="cuda")
    shapes = (("sums", (1, 32), torch.int64), ("pair_key", (1, 40), torch.int64), ("pair_d2", (1, 40), torch.int32), ("pair_normal", (1, 40), torch.int32))
    out = {k: torch.full(shape, 77, dtype=dt, device="cuda") for k, shape, dt in shapes}
    good = [buf.data_ptr(), nbytes, ctypes.byref(spec), xyz.data_ptr(), 0, n.data_ptr(), counts.data_ptr(), poses.data_ptr(), origin.data_ptr(), 1, 40, 65536, 1, 1, 0,
            normal.data_ptr(), slots, dirs.data_ptr(), 9] + [out[k].data_ptr() for k, _, _ in shapes] + [ws.data_ptr(), need.value, st]
    bad = {0: [None, buf.data_ptr() + 8], 1: [nbytes - 8, 0], 2: [None, spec_with(size=float("nan")), spec_with(capacity=2 ** 26 + 1), spec_with(lo=(2, float("-inf")))],
           3: [None, xyz.data_ptr() + 2], 4: [2, -1], 5: [n.data_ptr() + 2], 6: [None, counts.data_ptr() + 1], 7: [None, poses.data_ptr() + 4], 8: [None, origin.data_ptr() + 2],
           9: [-1, 65536], 10: [-1], 11: [-1, 783364], 15: [None, normal.data_ptr() + 2], 16: [slots - 1, 2 * slots], 17: [None, dirs.data_ptr() + 1], 18: [0, 4097],
           19: [None, out["sums"].data_ptr() + 4], 20: [None, out["pair_key"].data_ptr() + 4], 21: [None, out["pair_d2"].data_ptr() + 2], 22: [None, out["pair_normal"].data_ptr() + 2],
           23: [None, ws.data_ptr() + 4], 24: [need.value - 1, 0]}
    for at, values in bad.items():
        for v in values:
            assert L.sv_voxel_plane_align_device(*(good[:at] + [v] + good[at + 1:])) == SV_ERR_ARG and b"sv_voxel_plane_align" in L.sv_last_error(None), (at, v)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and all((t == 77).all().item() for t in out.values()) and (ws == 77).all().item()  # nothing was enqueued
    assert L.sv_voxel_plane_align_device(*(good[:3] + [None, 0, None, None, None, None, 0, 40, 65536, 1, 1, 0, None, 0, None, 9] + [None] * 4 + [None, 0, st])) == 0  # an empty batch needs no pointer
    assert L.sv_voxel_plane_align_device(*(good[:20] + [None, None, None] + good[23:])) == 0  # only the sums
    torch.cuda.synchronize()
    assert out["sums"][0, :5].tolist() == [40, 40, 40, 80, 0] and all((out[k] == 77).all().item() for k in PLANE_FIELDS[1:]) and (ws[-2:] == 77).all().item()
    assert L.sv_voxel_plane_align_device(*good) == 0
    torch.cuda.synchronize()
    assert out["pair_key"][0].tolist() == [key_of(c) for c in cases.distinct_cells(40)] and not out["pair_normal"].any().item() and torch.equal(buf, before)


@pytest.mark.gpu
def test_the_cli(sv, eng, tmp_path):
    from PIL import Image
    from test_occupancy_map import _drive_frames
    ls, rs = _drive_frames(2)
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    for i in range(2):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("0.0 0.0 0.0\n0.8 0.05 0.03\n")
    base = ["-k", str(tmp_path / "kitti"), "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt"), "--batch", "1"]
    plane = str(tmp_path / "plane.ply")
    sv.main(base + ["--voxel-map", plane, "--voxel-align", "3,1.5,4,plane"])  # frame 1 against frame 0
    lines = [[float(w) for w in line.split()] for line in open(os.path.splitext(plane)[0] + ".aligned.txt")]
    assert len(lines) == 2 and all(len(words) == 12 and np.isfinite(words).all() for words in lines)
    assert lines[0] == sv.voxel_map_pose(0.0, 0.0, 0.0).tolist() and lines[1][6:9] == [0.0, 0.0, 1.0]
    R = np.array(lines[1][:9]).reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.abs(np.array(lines[1][9:]) - (0.8, 0.05, 0.0)).max() < 1.0 and os.path.getsize(plane) > 1000
    for bad in ("3,1,6,planes", "3,1,6,plane,2"):
        with pytest.raises(SystemExit):
            sv.main(base + ["--voxel-map", plane, "--voxel-align", bad])
