"""A frame matched against the voxel map over candidate 3-D poses (group (R)): the numpy definition against hand numbers and a per-row
model, and the GPU (engine.voxel_map_match, rig.VoxelMap.match / .localize, the CLI) against the definition - shape, dtype and bits."""
import math
import os
import re

import numpy as np
import pytest

import util
import voxel_map_cases as cases
import voxel_match_cases as mcases
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_map_cases import BOX16, IDENTITY, PROBE_BOX, QUARTER
from voxel_match_cases import FIELDS, same, shifted

SV_ERR_ARG = -1
BOX4K = dict(BOX16, capacity=4096)  # BOX16 with room for all of its 4096 cells
HAND = dict(lo=(0.0, 0.0, -0.9), hi=(4.0, 4.0, 1.1), size=1.0, capacity=512)  # test_voxel_map's: 4 x 4 x 2 cells


def _define(sv, params, calls):
    state, seq = sv.voxel_map_state(sv.voxel_map_params(**params)), 0
    for call in calls:
        sv.voxel_map_insert(state, *call, seq0=seq)
        seq += call[0].shape[0]
    return state


def _hand_map(sv):
    """test_voxel_map's hand map: voxel a = cell (1, 2, 0) with n 5, m 2, S (5 * 32768, 0, 5 * 32768) and voxel b = cell (1, 2, 1) with n 5,
    m 1, S (5 * 32768, 5 * 16384, 5 * 65535)."""
    top = math.nextafter(1.1, 0.0)
    f0 = np.array([[2.0, -1.5, -0.4], [np.nan, 1.0, 0.0], [1.0, 0.0, -0.4]])
    f1 = np.array([[0.5, 2.25, top - 0.5], [0.5, 2.0, -0.9], [9.0, 9.0, 9.0]])
    n = np.array([[3, 1, 1], [5, 2, 1]], np.int32)
    state = _define(sv, HAND, [(np.stack([f0, f1]), None, n, np.array([3, 2], np.int32), np.stack([QUARTER, shifted((1.0, 0.0, 0.5))]))])
    assert state["key"].tolist() == [1 | 2 << 20, 1 | 2 << 20 | 1 << 40] and state["S"].tolist() == [[5 * 32768, 0, 5 * 32768], [5 * 32768, 5 * 16384, 5 * 65535]]
    return state


def _hand_frame():
    top = math.nextafter(1.1, 0.0)  # hi minus one ulp: t = 2.0, so the cell is clamped to 1 and u to 65535
    xyz = np.array([[[1.5, 2.0, -0.4],     # on a cell boundary in y: cell (1, 2, 0), u = (32768, 0, 32768) - voxel a's own mean
                     [2.0, -1.5, -0.4],    # the same point after the quarter turn (-y, x, z); outside under the identity
                     [1.25, 2.5, top]]])   # cell (1, 2, 1), u = (16384, 32768, 65535): 16384 off voxel b's mean on two axes
    return xyz, np.array([[1, 3, 2]], np.int32), np.array([3], np.int32), np.stack([IDENTITY, QUARTER, shifted((10.0, 0.0, 0.0))])[None]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_hand_case(sv):
    state = _hand_map(sv)
    xyz, n, counts, poses = _hand_frame()
    got = sv.voxel_map_match(state, xyz, n, counts, poses)
    assert got["inside"].tolist() == [[2, 1, 0]] and got["hits"].tolist() == [[2, 1, 0]] and got["inside"].dtype == got["hits"].dtype == np.int32
    assert got["weight"].tolist() == [[3, 3, 0]] and got["d2"].tolist() == [[2 * 16384 ** 2, 0, 0]] and got["weight"].dtype == got["d2"].dtype == np.int64
    assert got["best"].tolist() == [1] and got["best"].dtype == np.int32  # equal weights: the smaller d2 wins
    assert got["best_weight"].tolist() == [3] and got["best_d2"].tolist() == [0] and got["best_weight"].dtype == got["best_d2"].dtype == np.int64
    assert same(got, mcases.model_match(sv, state, xyz, n, counts, poses))
    settled = sv.voxel_map_match(state, xyz, n, counts, poses, min_rows=2)  # voxel b has one row: the row at hi - 1 ulp misses
    assert settled["inside"].tolist() == [[2, 1, 0]] and settled["hits"].tolist() == [[1, 1, 0]] and settled["weight"].tolist() == [[1, 3, 0]]
    assert settled["d2"].tolist() == [[0, 0, 0]] and settled["best"].tolist() == [1]
    f32 = sv.voxel_map_match(state, xyz.astype(np.float32), None, counts, poses[0])  # [P,12] for one frame; float32(top) is 1.1f > hi
    assert f32["inside"].tolist() == [[1, 1, 0]] and f32["weight"].tolist() == [[1, 1, 0]] and f32["best"].tolist() == [0]
    before = {k: np.copy(v) for k, v in state.items() if isinstance(v, np.ndarray)}
    sv.voxel_map_match(state, xyz, n, counts, poses)
    assert all(np.array_equal(state[k], v) for k, v in before.items())  # the map is not changed


def test_definition_against_model(sv):
    kinds, hit = set(), 0
    for seed in range(30):
        params, calls, (xyz, n, counts), poses, filters = mcases.random_match(seed)
        state = _define(sv, params, calls)
        got = sv.voxel_map_match(state, xyz, n, counts, poses, **filters)
        assert same(got, mcases.model_match(sv, state, xyz, n, counts, poses, **filters)), seed
        assert (got["inside"][:, 3] == 0).all() and (got["hits"] <= got["inside"]).all()  # the pose that is not finite keeps nothing
        kinds.add((str(xyz.dtype), n is None))
        hit += int(got["hits"].sum())
    assert len(kinds) == 4 and hit > 1000  # f32 and f64, with and without weights


def test_own_pose(sv):
    rng = np.random.default_rng(8)
    pts = cases.distinct_cells(200) + rng.uniform(0.01, 0.6, (200, 3))  # at most one row per cell, under the pose as well
    pts[7], pts[50] = np.nan, (20.0, 1.0, 1.0)
    pose = shifted((0.3, 0.2, 0.1))
    for dtype in (np.float64, np.float32):
        call = cases.one_frame(pts, None, None, pose, dtype)
        state = _define(sv, BOX16, [call])
        kept = 200 - state["dropped"]
        got = sv.voxel_map_match(state, call[0], None, call[3], np.stack([call[4][0], shifted((1.0, 0.0, 0.0), pose)])[None])
        assert 150 < kept < 199 and len(state["key"]) == kept
        assert got["inside"][0, 0] == got["hits"][0, 0] == got["weight"][0, 0] == kept and got["d2"][0, 0] == 0 and got["best"].tolist() == [0]
        assert 0 < got["hits"][0, 1] < got["inside"][0, 1] < kept and got["d2"][0, 1] > 0  # one cell on: the last column leaves the box, two rows find no voxel


def _scene_case(dtype):
    world, frame = mcases.scene()
    return cases.one_frame(world.copy(), None, None, IDENTITY, np.float64), (frame.astype(dtype)[None], None, np.array([len(frame)], np.int32))


def _true_candidate(sv):
    window = sv.voxel_map_pose_window(*mcases.SCENE_GUESS, *mcases.SCENE_WINDOW)
    at = int(np.abs(window - mcases.SCENE_TRUTH).sum(1).argmin())
    assert len(window) == 375 and np.abs(window[at] - mcases.SCENE_TRUTH).max() < 1e-12 and at != 0
    return window, at


def test_localisation(sv):
    window, at = _true_candidate(sv)
    for dtype in (np.float64, np.float32):
        call, (xyz, n, counts) = _scene_case(dtype)
        world = util.pkg("rig").VoxelMap(device="cpu", **mcases.SCENE_BOX)
        world.update(*call)
        refined, res = world.localize(xyz, n, counts, mcases.SCENE_GUESS, *mcases.SCENE_WINDOW)
        print("true candidate %d scores %d of %d; the runner-up %d" % (at, int(res.weight[0, at]), xyz.shape[1], int(np.sort(res.weight[0].numpy())[-2])))
        assert res.best.tolist() == [at] and refined.shape == (1, 4) and refined.dtype == np.float64 and np.array_equal(refined[0], window[at])
        assert world.stats() == {"claimed": len(world._state["key"]), "dropped": 0, "overflowed": False} and world.seq == 1  # unchanged by the match


def test_ties(sv):
    calls, xyz, counts, (off, exact, both, miss) = mcases.ties_case()
    state = _define(sv, BOX16, calls)
    got = sv.voxel_map_match(state, xyz, None, counts, np.stack([miss, off, exact, exact, both])[None])
    assert got["weight"].tolist() == [[0, 1, 1, 1, 2]] and got["d2"].tolist() == [[0, 16384 ** 2, 0, 0, 5 * 16384 ** 2]]
    assert got["best"].tolist() == [4] and got["best_weight"].tolist() == [2] and got["best_d2"].tolist() == [5 * 16384 ** 2]  # weight before d2
    got = sv.voxel_map_match(state, xyz, None, counts, np.stack([miss, off, exact, exact])[None])
    assert got["best"].tolist() == [2] and got["best_d2"].tolist() == [0]  # equal weight: the smaller d2, and of two such the lower p
    got = sv.voxel_map_match(state, xyz, None, counts, np.stack([miss, miss, miss])[None])
    assert got["best"].tolist() == [0] and got["best_weight"].tolist() == [0]  # nothing hits anywhere: candidate 0, the guess


def _overflowed(sv):
    params = dict(BOX16, capacity=2)
    return params, [cases.one_frame(cases.cell_points(cases.distinct_cells(3)))]


def test_overflowed_map(sv):
    params, calls = _overflowed(sv)
    state = _define(sv, params, calls)
    assert state["overflowed"]
    xyz, counts = calls[0][0], calls[0][3]
    got = sv.voxel_map_match(state, xyz, None, counts, np.stack([IDENTITY, IDENTITY])[None])
    assert same(got, {k: np.zeros((1, 2) if k in FIELDS[:4] else (1,), mcases.DTYPES[k]) - (k == "best") for k in FIELDS})
    world = util.pkg("rig").VoxelMap(device="cpu", **params)
    world.update(*calls[0])
    refined, res = world.localize(xyz, None, counts, [1.0, 2.0, 0.5, 0.1], (0.5, 0.5, 0.0, 0.0), (3, 3, 1, 1))
    assert res.best.tolist() == [-1] and refined.tolist() == [[1.0, 2.0, 0.5, 0.1]]  # the guess is kept


def test_filters(sv):
    calls, (xyz, n, counts) = mcases.filter_calls()
    state = _define(sv, BOX16, calls)
    full = sv.voxel_map_rows(state)
    assert full["n"].tolist() == [6, 12, 12, 8, 10, 12] and full["m"].tolist() == [3, 6, 6, 4, 5, 6] and full["last_seq"].tolist() == [2, 2, 1, 0, 0, 0]
    for kw, hits in ((dict(), 6), (dict(min_n=9), 4), (dict(min_n=10), 4), (dict(min_n=11), 3), (dict(min_rows=4), 5), (dict(min_rows=5), 4), (dict(min_rows=6), 3),
                     (dict(since=0), 6), (dict(since=1), 3), (dict(since=2), 2), (dict(since=3), 0), (dict(min_n=10, min_rows=5, since=1), 2)):
        got = sv.voxel_map_match(state, xyz, n, counts, IDENTITY[None, None], **kw)
        assert got["inside"].tolist() == [[6]] and got["hits"].tolist() == [[hits]] and got["weight"].tolist() == [[hits]], kw
        assert got["d2"].tolist() == [[hits * 3 * 16384 ** 2]] and same(got, mcases.model_match(sv, state, xyz, n, counts, IDENTITY[None, None], **kw)), kw


def test_refusals_and_the_window(sv, tmp_path):
    state = _define(sv, BOX16, [cases.one_frame(cases.cell_points([(3, 4, 5)]))])
    xyz, counts = np.zeros((1, 4, 3)), np.array([4], np.int32)
    for poses in (np.zeros((1, 0, 12)), np.zeros((1, 65536, 12)), np.zeros((1, 3, 4)), np.zeros((2, 3, 12)), np.zeros(12)):
        with pytest.raises(ValueError):
            sv.voxel_map_match(state, xyz, None, counts, poses)
    for kw in (dict(xyz=np.zeros((1, 4, 2))), dict(counts=np.zeros(2, np.int32)), dict(n=np.zeros((1, 3), np.int32))):
        with pytest.raises(ValueError):
            sv.voxel_map_match(state, **dict(dict(xyz=xyz, n=None, counts=counts, poses=IDENTITY[None, None]), **kw))
    assert sv.voxel_map_match(state, xyz, None, counts, np.zeros((1, 65535, 12)))["best"].tolist() == [0]  # the largest window there is
    empty = sv.voxel_map_match(state, np.zeros((0, 4, 3)), None, np.zeros(0, np.int32), np.zeros((0, 3, 12)))
    assert same(empty, {k: np.zeros((0, 3) if k in FIELDS[:4] else (0,), mcases.DTYPES[k]) for k in FIELDS})
    for half, steps in (((1, 1, 1, 1), (3, 2, 1, 1)), ((1, 1, 1, 1), (3, 3, 1, 0)), ((1, 1, 1), (3, 3, 3)), ((1, -1, 1, 1), (3, 3, 3, 3)),
                        ((1, 1, 1, np.inf), (3, 3, 3, 3)), ((1, 1, 1, 1), (41, 41, 39, 1)), ((1, 1, 1, 1), (3, 3, 1.5, 1))):
        with pytest.raises(ValueError):
            sv.voxel_map_pose_window(0.0, 0.0, 0.0, 0.0, half, steps)
    w = sv.voxel_map_pose_window(1.0, 2.0, 3.0, 0.5, (0.5, 1.0, 0.25, 0.1), (3, 5, 3, 1))
    assert w.shape == (45, 4) and w.dtype == np.float64 and w[0].tolist() == [1.0, 2.0, 3.0, 0.5] and len({tuple(r) for r in w.tolist()}) == 45
    assert w[1].tolist() == [0.5, 1.0, 2.75, 0.5] and w[2].tolist() == [0.5, 1.0, 3.0, 0.5] and w[-1].tolist() == [1.5, 3.0, 3.25, 0.5]  # row-major, yaw fastest
    assert sv.voxel_map_pose_window(1.0, 2.0, 3.0, 0.5, (9, 9, 9, 9), (1, 1, 1, 1)).tolist() == [[1.0, 2.0, 3.0, 0.5]]
    assert sv.voxel_map_pose_window(0, 0, 0, 0, (1, 1, 1, 1), (255, 257, 1, 1)).shape == (65535, 4)
    poses = sv.voxel_map_pose(w[:, 0], w[:, 1], w[:, 3], w[:, 2])
    assert poses.shape == (45, 12) and poses[0, 9:].tolist() == [1.0, 2.0, 3.0] and poses[0, 0] == math.cos(0.5) and poses[0, 3] == math.sin(0.5)
    cpu = util.pkg("rig").VoxelMap(device="cpu", **BOX16)  # rig.VoxelMap on CPU tensors runs the definition
    cpu.update(*cases.one_frame(cases.cell_points([(3, 4, 5)])))
    res = cpu.match(np.array([[[0.5, 0.5, 0.5]]]), None, np.array([1], np.int32), np.stack([IDENTITY, shifted((3.0, 4.0, 5.0))])[None])
    want = sv.voxel_map_match(state, np.array([[[0.5, 0.5, 0.5]]]), None, np.array([1], np.int32), np.stack([IDENTITY, shifted((3.0, 4.0, 5.0))])[None])
    assert same({k: getattr(res, k).numpy() for k in FIELDS}, want) and res.best.tolist() == [1] and res.__slots__ == FIELDS
    with pytest.raises(ValueError):
        cpu.localize(np.zeros((1, 1, 3)), None, np.array([1], np.int32), [0.0, 0.0, 0.0], (1, 1, 1, 1), (3, 3, 3, 3))  # a guess of three words
    poses_file, ply, out = str(tmp_path / "poses.txt"), str(tmp_path / "ply"), str(tmp_path / "drive.ply")
    with open(poses_file, "w") as f:
        f.write("0 0 0\n")
    full = ["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", ply, "--voxel", "0.2", "--poses", poses_file]
    for bad in (full + ["--voxel-match", "0.1,0.1,0.1,0.01"], full + ["--voxel-map", out, "--voxel-match", "0.1,0.1,0.1"],
                full + ["--voxel-map", out, "--voxel-match", "0.1,0.1,0.1,0.01,3,3,2,1"], full + ["--voxel-map", out, "--voxel-match", "0.1,0.1,x,0.01"]):
        with pytest.raises(SystemExit):
            sv.main(bad)
    assert not os.path.exists(out) and not os.path.exists(ply)


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z_]*voxel_match[a-z_]*)\s*\(", src))
    assert declared == {"sv_voxel_match_workspace", "sv_voxel_match_device", "sv_debug_voxel_match"}
    assert text.index("/* ---- (Q)") < text.index("/* ---- (R)") < text.index("/* ---- (A)") and " *  (R) " in text
    assert set(util.pkg("engine").STAGE_SIGNATURES["voxel_match"]) == declared
    build = util.pkg("build")
    assert "voxel_match_kernels.hip" in build.SOURCES and "voxel_match.cpp" in build.SOURCES and "voxel_match_kernels.h" in build.HEADERS
    assert all(n in sv.__doc__ for n in ("voxel_map_pose_window", "voxel_map_match")) and "(R)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_match_kernels.hip")).read()
    assert "asm" not in source and "atomic" not in source.replace("no atomics", "")  # plain loads and stores only
    # the cell rule, the offsets, slot_of and the probe are the map's own, defined once
    cases.check_map_table(build)
    assert all(source.count(call) == 1 for call in ("vmap_cell(", "vmap_offset(", "vmap_find(", "vmap_passes("))


# ---------------------------------------------------------------------------------------------------------------- GPU

def _engine_map(eng, sv, params, calls):
    words = sv.voxel_map_params(**params)
    buf, seq = eng.voxel_map_new(words), 0
    for call in calls:
        eng.voxel_map_insert(buf, words, *[None if a is None else _cuda(a) for a in call[:4]], call[4], seq0=seq)
        seq += call[0].shape[0]
    return buf, words


def _host(res):
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in FIELDS}


def _gpu(eng, buf, words, xyz, n, counts, poses, **kw):
    return _host(eng.voxel_map_match(buf, words, _cuda(xyz), None if n is None else _cuda(n), _cuda(counts), poses, **kw))


def _both(eng, sv, params, calls, xyz, n, counts, poses, **kw):
    """(the GPU's dict, the definition's) for one map and one batch of frames."""
    buf, words = _engine_map(eng, sv, params, calls)
    return _gpu(eng, buf, words, xyz, n, counts, poses, **kw), sv.voxel_map_match(_define(sv, params, calls), xyz, n, counts, poses, **kw)


@pytest.mark.gpu
def test_the_cpu_cases_on_the_device(sv, eng):
    xyz, n, counts, poses = _hand_frame()
    hand = [(np.stack([np.array([[2.0, -1.5, -0.4], [np.nan, 1.0, 0.0], [1.0, 0.0, -0.4]]), np.array([[0.5, 2.25, math.nextafter(1.1, 0.0) - 0.5], [0.5, 2.0, -0.9], [9.0, 9.0, 9.0]])]),
             None, np.array([[3, 1, 1], [5, 2, 1]], np.int32), np.array([3, 2], np.int32), np.stack([QUARTER, shifted((1.0, 0.0, 0.5))]))]
    for kw in (dict(), dict(min_rows=2)):
        got, want = _both(eng, sv, HAND, hand, xyz, n, counts, poses, **kw)
        assert same(got, want) and got["best"].tolist() == [1] and got["weight"].tolist() == [[3 if not kw else 1, 3, 0]]
    got, want = _both(eng, sv, HAND, hand, xyz.astype(np.float32), None, counts, poses[0])
    assert same(got, want) and got["inside"].tolist() == [[1, 1, 0]]
    hit = 0
    for seed in range(30):
        params, calls, (xyz, n, counts), poses, filters = mcases.random_match(seed)
        got, want = _both(eng, sv, params, calls, xyz, n, counts, poses, **filters)
        assert same(got, want), seed
        hit += int(got["hits"].sum())
    assert hit > 1000
    state, xyz, counts, (off, exact, both, miss) = mcases.ties_case()
    for poses, best in (([miss, off, exact, exact, both], 4), ([miss, off, exact, exact], 2), ([miss, miss, miss], 0), ([off, exact] + [miss] * 300 + [exact], 1)):
        got, want = _both(eng, sv, BOX16, state, xyz, None, counts, np.stack(poses)[None])
        assert same(got, want) and got["best"].tolist() == [best]
    calls, (xyz, n, counts) = mcases.filter_calls()
    buf, words = _engine_map(eng, sv, BOX16, calls)
    state = _define(sv, BOX16, calls)
    for kw in (dict(), dict(min_n=9), dict(min_n=10), dict(min_n=11), dict(min_rows=4), dict(min_rows=5), dict(min_rows=6), dict(since=0), dict(since=1), dict(since=2),
               dict(since=3), dict(min_n=10, min_rows=5, since=1)):
        assert same(_gpu(eng, buf, words, xyz, n, counts, IDENTITY[None, None], **kw), sv.voxel_map_match(state, xyz, n, counts, IDENTITY[None, None], **kw)), kw
    params, calls = _overflowed(sv)
    got, want = _both(eng, sv, params, calls, calls[0][0], None, calls[0][3], np.stack([IDENTITY, IDENTITY])[None])
    assert same(got, want) and got["best"].tolist() == [-1] and not got["inside"].any()


@pytest.mark.gpu
def test_row_and_candidate_counts(sv, eng):
    rng = np.random.default_rng(21)
    fill = [cases.one_frame(rng.uniform(0.0, 16.0, (3000, 3)), None, rng.integers(1, 9, 3000), dtype=np.float32)]
    buf, words = _engine_map(eng, sv, BOX4K, fill)
    state = _define(sv, BOX4K, fill)
    assert not state["overflowed"] and len(state["key"]) > 2000
    tile = 1024  # rows of a frame a workgroup of the score kernel holds: VMATCH_TILE
    assert "VMATCH_ROWS = 4" in open(os.path.join(util.pkg("build").CSRC, "voxel_match_kernels.h")).read()
    cand = lambda P: np.stack([shifted(rng.uniform(-0.6, 0.6, 3)) for _ in range(P)])[None]  # noqa: E731
    for rows in (1, 63, 64, 65, 255, 256, 257, tile + 1):  # a wavefront and a workgroup turn over
        xyz = rng.uniform(-1.0, 17.0, (1, rows, 3)).astype(np.float32 if rows % 2 else np.float64)
        n, counts, poses = rng.integers(-1, 9, (1, rows)).astype(np.int32), np.array([rows], np.int32), cand(3)
        got = _gpu(eng, buf, words, xyz, n, counts, poses)
        assert same(got, sv.voxel_map_match(state, xyz, n, counts, poses)) and (got["hits"].sum() > 0 or rows == 1), rows
    xyz, counts = rng.uniform(0.0, 16.0, (4, 257, 3)), np.array([-1, 0, 264, 100], np.int32)  # counts of -1, 0 and above cap
    poses = np.concatenate([cand(5) for _ in range(4)])
    got, want = _gpu(eng, buf, words, xyz, None, counts, poses), sv.voxel_map_match(state, xyz, None, counts, poses)
    assert same(got, want) and got["inside"][:, 0].tolist()[:2] == [0, 0] and got["best"].tolist()[:2] == [0, 0] and got["inside"][2].max() > 200
    big = rng.uniform(0.0, 16.0, (1, 66 * tile + 5, 3)).astype(np.float32)  # more tiles than row chunks: a workgroup takes two
    counts, poses = np.array([big.shape[1]], np.int32), cand(2)
    got = _gpu(eng, buf, words, big, None, counts, poses)
    assert same(got, sv.voxel_map_match(state, big, None, counts, poses)) and got["hits"].min() > 30000
    xyz, counts = rng.uniform(0.0, 16.0, (1, 300, 3)), np.array([300], np.int32)
    try:
        for group, counts_p in ((0, (1, 2, 65)), (1, (1, 2)), (8, (7, 8, 9)), (64, (65, 129))):  # one below, at and one above a chunk
            assert eng.debug_voxel_match(group) == 0
            for P in counts_p:
                poses = cand(P)
                got, want = _gpu(eng, buf, words, xyz, None, counts, poses), sv.voxel_map_match(state, xyz, None, counts, poses)
                assert same(got, want), (group, P)
                best = _gpu(eng, buf, words, xyz, None, counts, poses, want_sums=False)
                assert same(best, want, FIELDS[4:]) and all(best[k] is None for k in FIELDS[:4])
        poses, seen = cand(37), []
        for group in (0, 1, 2, 4, 16, 64):  # the outputs do not depend on the hook
            eng.debug_voxel_match(group)
            seen.append(_gpu(eng, buf, words, xyz, None, counts, poses))
        assert all(same(s, seen[0]) for s in seen) and same(seen[0], sv.voxel_map_match(state, xyz, None, counts, poses))
        assert eng.debug_voxel_match(3) == SV_ERR_ARG and eng.debug_voxel_match(128) == SV_ERR_ARG and eng.debug_voxel_match(-1) == SV_ERR_ARG
    finally:
        eng.debug_voxel_match(0)


@pytest.mark.gpu
def test_probe_chains(sv, eng):
    for slot in (500, 1023):  # colliding keys; from the last slot the probes wrap to slots 0 .. 6
        cells = cases.colliding_cells(sv.voxel_map_slot_of, slot, 9)
        key = cells[:, 0] | (cells[:, 1] << 20) | (cells[:, 2] << 40)
        assert (sv.voxel_map_slot_of(key, 1024) == slot).all()
        calls = [cases.one_frame(cases.cell_points(cells[:8]), dtype=np.float32)]  # a chain of eight; the ninth cell is not in the map
        buf, words = _engine_map(eng, sv, PROBE_BOX, calls)
        state = _define(sv, PROBE_BOX, calls)
        chain = eng.voxel_map_rows(buf, words, sort=False)["key"][:8].cpu().numpy()  # in slot order - for slot 1023 the wrapped ones first
        if slot == 1023:
            chain = np.roll(chain, 1)
        assert sorted(chain.tolist()) == sorted(key[:8].tolist())
        by_key = {int(k): c for k, c in zip(key, cells)}
        first, middle, last = (cases.cell_points([by_key[int(chain[i])]], 0.25) for i in (0, 4, 7))
        absent = cases.cell_points([cells[8]], 0.25)  # its chain passes all eight foreign keys and ends at an empty slot
        for rows, hits in ((first, 1), (middle, 1), (last, 1), (absent, 0), (np.concatenate([first, middle, last, absent]), 3), (cases.cell_points(cells, 0.75), 8)):
            xyz, counts = rows[None], np.array([len(rows)], np.int32)
            got, want = _gpu(eng, buf, words, xyz, None, counts, IDENTITY[None, None]), sv.voxel_map_match(state, xyz, None, counts, IDENTITY[None, None])
            assert same(got, want) and got["hits"].tolist() == [[hits]] and got["inside"].tolist() == [[len(rows)]] and got["d2"].tolist() == [[hits * 3 * 16384 ** 2]]


@pytest.mark.gpu
def test_largest_payload(sv, eng):
    params, calls, _ = cases.painted_cases()["largest_payload"]
    one_more = cases.one_frame(cases.cell_points([(15, 15, 15)], 0.0))  # u = 0, weight 1: n is odd, S / n leaves a remainder
    xyz = np.concatenate([cases.cell_points([(15, 15, 15)], 0.0), cases.cell_points([(15, 15, 15)], 1.0 - 2.0 ** -20)])[None]  # u = 0 and u = 65535
    counts, poses = np.array([2], np.int32), IDENTITY[None, None]
    for fill, mean in ((calls, 65535), (calls + [one_more], 65534)):
        state = _define(sv, params, fill)
        assert state["n"].tolist() == [64 * (2 ** 31 - 1) + len(fill) - 1] and state["S"][0, 0] > 2 ** 52 and state["S"][0, 0] // state["n"][0] == mean
        got, want = _both(eng, sv, params, fill, xyz, None, counts, poses)
        assert same(got, want) and got["hits"].tolist() == [[2]] and got["d2"].tolist() == [[3 * mean ** 2 + 3 * (65535 - mean) ** 2]]
        heavy = np.full((1, 2), 2 ** 31 - 1, np.int32)
        got, want = _both(eng, sv, params, fill, xyz, heavy, counts, poses)
        assert same(got, want) and got["weight"].tolist() == [[2 * (2 ** 31 - 1)]]


@pytest.mark.gpu
def test_rows_that_drop(sv, eng):
    rng = np.random.default_rng(4)
    fill = [cases.one_frame(cases.cell_points(cases.distinct_cells(512)), dtype=np.float32)]  # the two bottom layers of BOX16, full
    buf, words = _engine_map(eng, sv, BOX16, fill)
    state = _define(sv, BOX16, fill)
    xyz = np.stack([rng.uniform(0.1, 15.9, 12), rng.uniform(0.1, 15.9, 12), rng.uniform(0.1, 1.9, 12)], -1)
    n = np.full(12, 2, np.int32)
    xyz[0, 0], xyz[1, 1], xyz[2, 2], xyz[3] = np.nan, np.inf, -np.inf, np.nan
    n[4], n[5] = 0, -1
    xyz[6, 0], xyz[7, 1], xyz[8, 2] = 0.0, 16.0, 0.0  # on lo, on hi, on lo
    xyz[9, 2] = 2.0 ** -100                           # just inside, as a float32 as well
    nan_pose, far, up = IDENTITY.copy(), shifted((0.0, 100.0, 0.0)), shifted((0.0, 0.0, 13.0))  # up: above the two layers, the row on lo in z inside
    nan_pose[4] = np.nan
    poses = np.stack([IDENTITY, nan_pose, far, up, shifted((0.0, 0.0, np.inf))])[None]
    for dtype in (np.float64, np.float32):
        rows = xyz.astype(dtype)[None]
        got, want = _gpu(eng, buf, words, rows, n[None], np.array([12], np.int32), poses), sv.voxel_map_match(state, rows, n[None], np.array([12], np.int32), poses)
        assert same(got, want)
        assert got["inside"].tolist() == [[3, 0, 0, 4, 0]] and got["hits"].tolist() == [[3, 0, 0, 0, 0]] and got["weight"].tolist() == [[6, 0, 0, 0, 0]]
    got = _gpu(eng, buf, words, xyz[None], None, np.array([12], np.int32), poses)  # without weights the rows of weight 0 and -1 count
    assert same(got, sv.voxel_map_match(state, xyz[None], None, np.array([12], np.int32), poses)) and got["inside"].tolist() == [[5, 0, 0, 6, 0]]


@pytest.mark.gpu
def test_read_only_and_batches(sv, eng):
    import torch
    rng = np.random.default_rng(6)
    fill = [cases.one_frame(rng.uniform(0.0, 16.0, (2000, 3)), rng.integers(0, 256, (2000, 4)), rng.integers(1, 5, 2000))]
    buf, words = _engine_map(eng, sv, BOX4K, fill)
    state = _define(sv, BOX4K, fill)
    before = buf.clone()
    xyz, n, counts = rng.uniform(-1.0, 17.0, (3, 400, 3)).astype(np.float32), rng.integers(0, 5, (3, 400)).astype(np.int32), np.array([400, 7, 130], np.int32)
    poses = np.stack([np.stack([shifted(rng.uniform(-1, 1, 3)) for _ in range(11)]) for _ in range(3)])
    got = _gpu(eng, buf, words, xyz, n, counts, poses)
    assert same(got, sv.voxel_map_match(state, xyz, n, counts, poses)) and all(a > b for a, b in zip(got["inside"].max(1).tolist(), (200, 2, 60)))
    on_device = eng.voxel_map_match(buf, words, _cuda(xyz), _cuda(n), _cuda(counts), _cuda(poses))  # poses as a tensor
    assert same(_host(on_device), got) and isinstance(on_device, eng.VoxelMatchResult) and on_device.weight.device == buf.device
    for b in range(3):  # every frame alone
        alone = _gpu(eng, buf, words, xyz[b:b + 1], n[b:b + 1], counts[b:b + 1], poses[b])
        assert same(alone, {k: v[b:b + 1] for k, v in got.items()})
    none = _gpu(eng, buf, words, np.zeros((0, 400, 3), np.float32), None, np.zeros(0, np.int32), np.zeros((0, 11, 12)))
    assert same(none, sv.voxel_map_match(state, np.zeros((0, 400, 3), np.float32), None, np.zeros(0, np.int32), np.zeros((0, 11, 12))))
    no_rows = _gpu(eng, buf, words, np.zeros((2, 0, 3)), None, np.array([0, 5], np.int32), poses[:2])  # cap 0: no score kernel, every output written
    assert same(no_rows, sv.voxel_map_match(state, np.zeros((2, 0, 3)), None, np.array([0, 5], np.int32), poses[:2])) and no_rows["best"].tolist() == [0, 0]
    torch.cuda.synchronize()
    assert torch.equal(buf, before)  # byte for byte
    for kw in (dict(xyz=_cuda(xyz).cpu()), dict(xyz=_cuda(xyz).half()), dict(counts=_cuda(counts).long()), dict(n=_cuda(n)[:, :3]), dict(poses=np.zeros((3, 11, 4))),
               dict(poses=np.zeros((2, 11, 12))), dict(poses=np.zeros((3, 0, 12))), dict(poses=_cuda(poses).float()), dict(min_n=0.5), dict(since=2 ** 31)):
        args = dict(dict(xyz=_cuda(xyz), n=_cuda(n), counts=_cuda(counts), poses=poses), **kw)
        with pytest.raises(ValueError):
            eng.voxel_map_match(buf, words, **args)
    with pytest.raises(ValueError):
        eng.voxel_map_match(buf[:100], words, _cuda(xyz), _cuda(n), _cuda(counts), poses)


@pytest.mark.gpu
def test_the_c_entry_refuses(sv, eng):
    import ctypes
    import torch
    words = sv.voxel_map_params(**BOX16)
    buf, _ = _engine_map(eng, sv, BOX16, [cases.one_frame(cases.cell_points(cases.distinct_cells(40)), dtype=np.float32)])
    before = buf.clone()
    xyz, n, counts = _cuda(cases.cell_points(cases.distinct_cells(40)).astype(np.float32)[None]), _cuda(np.full((1, 40), 2, np.int32)), _cuda(np.array([40], np.int32))
    poses = _cuda(np.stack([IDENTITY, shifted((1.0, 0.0, 0.0)), shifted((0.0, 1.0, 0.0))])[None])
    L = eng.voxel_match_lib()
    spec, nbytes, st = eng.voxel_map_spec(words), buf.numel() * 8, torch.cuda.current_stream().cuda_stream
    need = ctypes.c_size_t(7)
    for cap, P, B in ((-1, 3, 1), (40, 0, 1), (40, 65536, 1), (40, 3, -1), (40, 3, 65536), (40, 65535, 32769)):
        assert L.sv_voxel_match_workspace(cap, P, B, ctypes.byref(need)) == SV_ERR_ARG and need.value == 7 and b"sv_voxel_match" in L.sv_last_error(None)
    assert L.sv_voxel_match_workspace(40, 3, 1, None) == SV_ERR_ARG
    assert L.sv_voxel_match_workspace(40, 3, 1, ctypes.byref(need)) == 0 and need.value == (1 * 1 * 3 * 3 * 8 + 15) // 16 * 16 + 1 * 256 * 24  # one chunk
    assert L.sv_voxel_match_workspace(0, 3, 0, ctypes.byref(need)) == 0 and need.value == 0
    assert L.sv_voxel_match_workspace(64 * 1024 + 1, 5, 2, ctypes.byref(need)) == 0 and need.value == 2 * 64 * 3 * 5 * 8 + 2 * 256 * 24  # at most 64 chunks
    assert L.sv_voxel_match_workspace(40, 3, 1, ctypes.byref(need)) == 0
    ws = torch.full((need.value // 8 + 2,), 77, dtype=torch.int64, device="cuda")
    shapes = (("inside", (1, 3), torch.int32), ("hits", (1, 3), torch.int32), ("weight", (1, 3), torch.int64), ("d2", (1, 3), torch.int64), ("best", (1,), torch.int32),
              ("best_weight", (1,), torch.int64), ("best_d2", (1,), torch.int64))
    out = {k: torch.full(shape, 77, dtype=dt, device="cuda") for k, shape, dt in shapes}

    def spec_with(**kw):
        s = eng.voxel_map_spec(words)
        for k, v in kw.items():
            if k in ("lo", "hi", "reserved"):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return ctypes.byref(s)

    good = [buf.data_ptr(), nbytes, ctypes.byref(spec), xyz.data_ptr(), 0, n.data_ptr(), counts.data_ptr(), poses.data_ptr(), 1, 40, 3, 1, 1, 0] + \
        [out[k].data_ptr() for k, _, _ in shapes] + [ws.data_ptr(), need.value, st]
    bad = {0: [None, buf.data_ptr() + 8], 1: [nbytes - 8, 0],
           2: [None, spec_with(size=0.0), spec_with(size=float("nan")), spec_with(capacity=0), spec_with(capacity=2 ** 26 + 1), spec_with(reserved=(3, 1)),
               spec_with(hi=(1, 0.0)), spec_with(lo=(2, float("-inf"))), spec_with(size=1e-6)],
           3: [None, xyz.data_ptr() + 2], 4: [2, -1], 5: [n.data_ptr() + 2], 6: [None, counts.data_ptr() + 1], 7: [None, poses.data_ptr() + 4], 8: [-1, 65536], 9: [-1],
           10: [0, -1, 65536], 14: [None, out["inside"].data_ptr() + 2], 15: [None, out["hits"].data_ptr() + 1], 16: [None, out["weight"].data_ptr() + 4],
           17: [None, out["d2"].data_ptr() + 4], 18: [None, out["best"].data_ptr() + 2], 19: [None, out["best_weight"].data_ptr() + 4],
           20: [None, out["best_d2"].data_ptr() + 4], 21: [None, ws.data_ptr() + 8], 22: [need.value - 1, 0]}
    for at, values in bad.items():
        for v in values:
            assert L.sv_voxel_match_device(*(good[:at] + [v] + good[at + 1:])) == SV_ERR_ARG and b"sv_voxel_match" in L.sv_last_error(None), (at, v)
    assert L.sv_voxel_match_device(*(good[:8] + [32769, 40, 65535] + good[11:])) == SV_ERR_ARG  # batch x n_poses >= 2^31
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and all((t == 77).all().item() for t in out.values()) and (ws == 77).all().item()  # nothing was enqueued
    assert L.sv_voxel_match_device(*(good[:14] + [None] * 4 + good[18:])) == 0  # only the best
    torch.cuda.synchronize()
    assert out["best"].tolist() == [0] and out["best_weight"].tolist() == [80] and all((out[k] == 77).all().item() for k in FIELDS[:4]) and (ws[-2:] == 77).all().item()
    assert L.sv_voxel_match_device(*good) == 0  # and the good call goes through
    assert L.sv_voxel_match_device(*(good[:3] + [None, 0, None, None, None, 0, 40, 3, 1, 1, 0] + [None] * 7 + [None, 0, st])) == 0  # an empty batch needs no pointer
    torch.cuda.synchronize()
    assert out["inside"].tolist() == [[40, 38, 40]] and out["hits"].tolist() == [[40, 37, 24]] and out["weight"].tolist() == [[80, 74, 48]] and torch.equal(buf, before)


@pytest.mark.gpu
def test_the_classes_and_the_cli(sv, eng, tmp_path):
    from PIL import Image
    from test_occupancy_map import _drive_frames
    rigmod = util.pkg("rig")
    window, at = _true_candidate(sv)
    for dtype in (np.float64, np.float32):
        call, (xyz, n, counts) = _scene_case(dtype)
        worlds = [rigmod.VoxelMap(device=d, **mcases.SCENE_BOX) for d in ("cuda", "cpu")]
        worlds[0].update(*[None if a is None else _cuda(a) for a in call[:4]], call[4])
        worlds[1].update(*call)
        poses = sv.voxel_map_pose(window[:, 0], window[:, 1], window[:, 3], window[:, 2])[None]
        got, want = worlds[0].match(_cuda(xyz), None, _cuda(counts), poses), worlds[1].match(xyz, None, counts, poses)
        assert same(_host(got), _host(want)) and got.best.is_cuda and got.best.tolist() == [at]
        (refined, res), (refined_cpu, res_cpu) = (w.localize(x, None, c, mcases.SCENE_GUESS, *mcases.SCENE_WINDOW) for w, x, c in
                                                   ((worlds[0], _cuda(xyz), _cuda(counts)), (worlds[1], xyz, counts)))
        assert np.array_equal(refined, refined_cpu) and np.array_equal(refined[0], window[at]) and same(_host(res), _host(res_cpu)) and same(_host(res), _host(got))
        settled = worlds[0].match(_cuda(xyz), None, _cuda(counts), poses, min_rows=2, since=0)
        assert same(_host(settled), _host(worlds[1].match(xyz, None, counts, poses, min_rows=2, since=0))) and int(settled.hits.sum()) < int(got.hits.sum())
    params, calls = _overflowed(sv)
    over = rigmod.VoxelMap(device="cuda", **params)
    over.update(*[None if a is None else _cuda(a) for a in calls[0][:4]], calls[0][4])
    refined, res = over.localize(_cuda(calls[0][0]), None, _cuda(calls[0][3]), [1.0, 2.0, 0.5, 0.1], (0.5, 0.5, 0.0, 0.0), (3, 3, 1, 1))
    assert res.best.tolist() == [-1] and refined.tolist() == [[1.0, 2.0, 0.5, 0.1]] and not res.weight.any().item()
    # the CLI: two frames of the committed drive, the second matched against the first
    ls, rs = _drive_frames(2)
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    for i in range(2):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("0.0 0.0 0.0\n0.8 0.05 0.03\n")
    base = ["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt")]
    one, three = (str(tmp_path / name) for name in ("one.ply", "three.ply"))
    sv.main(base + ["--voxel-map", one, "--voxel-match", "0.2,0.2,0.2,0.02,1,1,1,1"])  # a window of the guess alone
    sv.main(base + ["--voxel-map", three, "--voxel-match", "0.2,0,0,0,3,1,1,1"])
    assert open(str(tmp_path / "one.poses.txt")).read() == "0.0 0.0 0.0 0.0\n0.8 0.05 0.0 0.03\n"
    lines = [[float(w) for w in line.split()] for line in open(str(tmp_path / "three.poses.txt"))]
    assert len(lines) == 2 and lines[0] == [0.0, 0.0, 0.0, 0.0] and lines[1][1:] == [0.05, 0.0, 0.03] and lines[1][0] in (0.8 - 0.2, 0.8, 0.8 + 0.2)
    assert os.path.getsize(one) > 1000 and os.path.getsize(three) > 1000
    with pytest.raises(SystemExit):
        sv.main(base + ["--voxel-match", "0.2,0,0,0,3,1,1,1"])
