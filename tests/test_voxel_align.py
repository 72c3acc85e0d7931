"""A frame aligned to the voxel map in six degrees of freedom (group (X)): the numpy definition of the sums of one round of iterative closest
point against hand numbers and a per-row model, the fit and the loop on a scene, and the GPU (engine.voxel_map_align_sums /
voxel_map_align, rig.VoxelMap.align, the CLI) against the definition - shape, dtype and bits."""
import os
import re

import numpy as np
import pytest

import util
import voxel_align_cases as acases
import voxel_map_cases as cases
import voxel_match_cases as mcases
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_align_cases import FIELDS, HAND, define, key_of, same
from voxel_map_cases import BOX16, IDENTITY, PROBE_BOX
from voxel_match_cases import shifted

SV_ERR_ARG = -1
BOX4K = dict(BOX16, capacity=4096)  # BOX16 with room for all of its 4096 cells
ZERO = np.zeros((1, 3), np.int32)


def _model_agrees(sv, state, frame, poses, origin, **kw):
    got = sv.voxel_map_align_sums(state, *frame, poses, origin, **kw)
    assert same(got, sv.voxel_map_align_sums_brute(state, *frame, poses, origin, **kw)), kw
    return got


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_hand_case(sv):
    """In 1/256 of a cell voxel a stands at (384, 512, 128), b at (384, 576, 511), c at (896, 512, 128).  No row can be as far from a as
    from b - (pz - 128)^2 and (pz - 511)^2 differ in parity and the other terms do not - so the tie is between a and c, which
    voxel_align_cases.hand_calls adds: the row at (640, 512, 128) is 256^2 = 65536 = max_d2 from both, and a has the smaller key."""
    state = define(sv, HAND, acases.hand_calls())
    a, b, c = key_of((1, 2, 0)), key_of((1, 2, 1)), key_of((3, 2, 0))
    assert state["key"].tolist() == [a, c, b] and state["S"].tolist() == [[5 * 32768, 0, 5 * 32768], [32768, 0, 32768], [5 * 32768, 5 * 16384, 5 * 65535]]
    before = {k: np.copy(v) for k, v in state.items() if isinstance(v, np.ndarray)}
    xyz, n, counts = acases.hand_frame()
    origin = np.array([[100, 200, -50]], np.int32)
    got = _model_agrees(sv, state, (xyz, n, counts), IDENTITY[None], origin)
    assert got["pair_key"].tolist() == [[a, a, a, -1, -1, b]] and got["pair_d2"].tolist() == [[0, 65536, 320 ** 2 + 192 ** 2, -1, -1, 2 * 64 ** 2]]
    assert got["sums"].shape == (1, 19) and got["sums"].dtype == np.int64 and got["pair_key"].shape == (1, 6) and got["pair_key"].dtype == np.int64
    assert got["pair_d2"].shape == (1, 6) and got["pair_d2"].dtype == np.int32
    # the pairs: (weight, p - o, q - o, d2) of rows 0, 1 and 5; row 2 is kept, and its nearest voxel is beyond max_d2
    pairs = [(1, (284, 312, 178), (284, 312, 178), 0), (3, (540, 312, 178), (284, 312, 178), 65536), (2, (220, 440, 561), (284, 376, 561), 8192)]
    want = [4, 3, 6, 3 * 65536 + 2 * 8192, 2344, 2128, 1834, 1704, 2000, 1834]
    want += [sum(w * p[i] * q[j] for w, p, q, _ in pairs) for i in range(3) for j in range(3)]
    assert want[10] == 284 * 284 + 3 * 540 * 284 + 2 * 220 * 284 == 665696 and want[11] == 284 * 312 + 3 * 540 * 312 + 2 * 220 * 376 == 759488
    assert want[4:7] == [sum(w * p[k] for w, p, _, _ in pairs) for k in range(3)] and want[7:10] == [sum(w * q[k] for w, _, q, _ in pairs) for k in range(3)]
    assert got["sums"].tolist() == [want]
    half = _model_agrees(sv, state, (xyz, n, counts), IDENTITY[None], origin, max_dist=0.5)  # max_d2 = 16384: rows 0 and 5 pair, the per-row words stay
    assert half["sums"][0, :4].tolist() == [4, 2, 3, 2 * 8192] and same(half, got, FIELDS[1:])
    settled = _model_agrees(sv, state, (xyz, n, counts), IDENTITY[None], origin, min_rows=2)  # a alone has two rows
    assert settled["pair_key"].tolist() == [[a, a, a, -1, -1, a]] and settled["sums"][0, :2].tolist() == [4, 2]
    four = sv.voxel_map_align_sums(state, xyz, n, counts, np.array([[0.0, 0.0, 1.0, 0.0]]), origin)  # [B,4] = (tx, ty, c, s)
    assert same(four, got)
    assert all(np.array_equal(state[k], v) for k, v in before.items())  # the map is not changed


def test_definition_against_model(sv):
    kinds, pairs, elsewhere = set(), 0, 0
    for seed in range(30):
        params, calls, frame, variants, origin, max_dist, filters = acases.random_align(seed)
        state = define(sv, params, calls)
        for v, poses in enumerate(variants):
            got = _model_agrees(sv, state, frame, poses, origin, max_dist=max_dist, **filters)
            assert (got["sums"][1] == 0).all() and (got["pair_key"][1] == -1).all()  # a count of 0 or -1
            assert v < 3 or (not got["sums"].any() and (got["pair_key"] == -1).all())  # the pose that is not finite keeps nothing
            assert (got["sums"][:, 1] <= got["sums"][:, 0]).all() and (got["sums"][:, 2] >= got["sums"][:, 1]).all()
            pairs += int(got["sums"][:, 1].sum())
            if v == 0:  # the row's own cell, from the rows' keys under the frame's pose
                xyz, n, counts = frame
                for i in range(min(int(counts[0]), xyz.shape[1])):
                    r = cases.row_key(params, xyz[0, i], [float(w) for w in poses[0]], 1 if n is None else int(n[0, i]))
                    assert r is not None or got["pair_key"][0, i] == -1  # a row that is not kept has no partner
                    elsewhere += r is not None and got["pair_key"][0, i] not in (-1, r[0])
        kinds.add((str(frame[0].dtype), frame[1] is None, max_dist))
    assert len({k[:2] for k in kinds}) == 4 and {k[2] for k in kinds} == set(acases.MAX_DISTS)  # f32 and f64, with and without weights
    assert pairs > 1000 and elsewhere > 0


def test_edges_of_the_box(sv):
    params, calls, frame = acases.edge_case()
    state = define(sv, params, calls)
    origin = sv.voxel_align_origin(state["params"], shifted((8.0, 8.0, 8.0))[None])
    assert origin.tolist() == [[2048, 2048, 2048]] and origin.dtype == np.int32
    for max_dist in (1.0, 2.0):
        got = _model_agrees(sv, state, frame, IDENTITY[None], origin, max_dist=max_dist)
        assert got["sums"][0, 0] == frame[0].shape[1] and got["sums"][0, 1] > 20 and (got["pair_key"] >= 0).all()  # every row has a voxel within a cell
    far = define(sv, BOX16, [cases.one_frame(cases.cell_points([(8, 8, 8)]))])  # a table with empty slots and no voxel near the corner
    corner = (np.array([[[0.5, 0.5, 0.5], [15.5, 15.5, 15.5], [0.5, 15.5, 0.5]]]), None, np.array([3], np.int32))
    got = _model_agrees(sv, far, corner, IDENTITY[None], ZERO, max_dist=2.0)
    assert got["sums"][0].tolist() == [3] + [0] * 18 and (got["pair_key"] == -1).all() and (got["pair_d2"] == -1).all()  # no partner "at" cell -1
    params, calls, frame = acases.long_case()  # cell 2^20 on x is no cell: its key would be cell (0, 1, 0)'s
    got = _model_agrees(sv, define(sv, params, calls), frame, IDENTITY[None], np.array([[2 ** 28 - 512, 0, 0]], np.int32), max_dist=2.0)
    assert got["pair_key"].tolist() == [[key_of((2 ** 20 - 2, 0, 0))] * 3 + [key_of((0, 1, 0))]] and got["sums"][0, :2].tolist() == [4, 4]


def test_tombstones(sv):
    params, calls, carve, frame = acases.tombstone_case()
    for also in (False, True):  # the neighbour stays, or is emptied as well
        state = define(sv, params, calls)
        res = sv.voxel_map_carve(state, **carve, apply=True)
        if also:
            res = sv.voxel_map_carve(state, np.array([[[6.5, 9.5, 5.5]]]), None, carve["counts"], carve["poses"], origin=(6.5, 2.5, 5.5), seq0=1, apply=True)
        assert res["carved"] == 1 and state["n"].tolist() == [0, 0 if also else 1] and len(state["key"]) == 2
        for kw in (dict(min_n=1), dict(min_n=0), dict(min_n=0, min_rows=0, since=-5), dict(min_n=-3, min_rows=-3, since=-2 ** 31)):
            got = _model_agrees(sv, state, frame, IDENTITY[None], ZERO, **kw)
            if also:
                assert got["sums"][0].tolist() == [1] + [0] * 18 and got["pair_key"].tolist() == [[-1]]
            else:
                assert got["pair_key"].tolist() == [[key_of((6, 5, 5))]] and got["pair_d2"].tolist() == [[256 ** 2]] and got["sums"][0, :4].tolist() == [1, 1, 1, 65536]
                assert sv.voxel_map_align_sums(state, *frame, IDENTITY[None], ZERO, max_dist=0.5, **kw)["sums"][0, :2].tolist() == [1, 0]


def _own_pose_case(sv, dtype):
    rng = np.random.default_rng(8)
    pts = cases.distinct_cells(200) + rng.uniform(0.01, 0.6, (200, 3))  # at most one row per cell, under the pose as well
    pts[7], pts[50] = np.nan, (20.0, 1.0, 1.0)
    return cases.one_frame(pts, None, None, shifted((0.3, 0.2, 0.1)), dtype)


def test_own_pose(sv):
    for dtype in (np.float64, np.float32):
        call = _own_pose_case(sv, dtype)
        state = define(sv, BOX16, [call])
        kept = 200 - state["dropped"]
        xyz, counts, pose = call[0], call[3], call[4]
        origin = sv.voxel_align_origin(state["params"], pose)
        got = sv.voxel_map_align_sums(state, xyz, None, counts, pose, origin)
        assert 150 < kept < 199 and got["sums"][0, :4].tolist() == [kept, kept, kept, 0]
        keys = [cases.row_key(BOX16, xyz[0, i], [float(v) for v in pose[0]], 1) for i in range(200)]
        assert got["pair_key"][0].tolist() == [-1 if r is None else r[0] for r in keys] and set(got["pair_d2"][0].tolist()) == {0, -1}
        new, ok, step = sv.voxel_align_solve(got["sums"], pose, origin, state["params"])
        assert ok.tolist() == [True] and new.shape == (1, 12) and new.dtype == np.float64 and np.abs(new - pose).max() < 1e-12 and step.shape == (1, 2) and step.max() < 1e-12
        new, ok, _ = sv.voxel_align_solve(got["sums"], pose, origin, state["params"], dof=4)
        assert ok.tolist() == [True] and np.abs(new - pose).max() < 1e-12


def _scene_state(sv):
    return define(sv, mcases.SCENE_BOX, [acases.scene_case()[0]])


def test_convergence(sv):
    state = _scene_state(sv)
    assert len(state["key"]) == 978
    frame, truth = acases.scene_case()[1], acases.scene_truth(sv)
    start = acases.scene_start(sv, *acases.SCENE_STARTS["all"])
    rot0, tr0 = acases.pose_error(start, truth)
    assert 2.6 < rot0 < 2.8 and 0.14 < tr0 < 0.15
    res = sv.voxel_map_align(state, *frame, start[None], iterations=15, max_dist=1.0, dof=6)
    rot, tr = acases.pose_error(res["poses"][0], truth)
    print("dof 6: %.4f deg, %.4f m -> %.4f deg, %.4f m in %d rounds, pairs %s" % (rot0, tr0, rot, tr, res["rounds"], res["pairs"][:, 0].tolist()))
    assert rot < rot0 / 10 and tr < tr0 / 10 and res["ok"].tolist() == [True] and res["pairs"][-1, 0] == 600 and res["sums"][0, 1] == 600
    assert 1 <= res["rounds"] <= 15 and res["pairs"].shape == res["rms"].shape == (res["rounds"], 1) and res["rms"][-1, 0] < res["rms"][0, 0]
    assert int(np.abs(res["sums"]).max()) < 2 ** 35
    yaw_only = sv.voxel_map_align(state, *frame, start[None], iterations=15, max_dist=1.0, dof=4)
    rot4, tr4 = acases.pose_error(yaw_only["poses"][0], truth)
    print("dof 4 on the same start: -> %.4f deg, %.4f m" % (rot4, tr4))
    assert rot4 > 1.0  # roll and pitch stay
    assert np.array_equal(yaw_only["poses"][0, 6:9], start[6:9])  # a turn about the world's z leaves the rotation's third row as it was
    start = acases.scene_start(sv, *acases.SCENE_STARTS["yaw"])
    rot0, tr0 = acases.pose_error(start, truth)
    res = sv.voxel_map_align(state, *frame, start[None], iterations=15, max_dist=1.0, dof=4)
    rot, tr = acases.pose_error(res["poses"][0], truth)
    print("dof 4 on a start off in yaw and translation: %.4f deg, %.4f m -> %.4f deg, %.4f m" % (rot0, tr0, rot, tr))
    assert rot < rot0 / 10 and tr < tr0 / 10 and res["pairs"][-1, 0] == 600
    cpu = util.pkg("rig").VoxelMap(device="cpu", **mcases.SCENE_BOX)  # rig.VoxelMap on CPU tensors runs the definition
    cpu.update(*acases.scene_case()[0])
    poses, result = cpu.align(*frame, start[None], iterations=15, dof=4)
    assert np.array_equal(poses, res["poses"]) and result.rounds == res["rounds"] and np.array_equal(result.sums.numpy(), res["sums"]) and poses.dtype == np.float64
    assert cpu.stats()["claimed"] == 978 and cpu.seq == 1  # unchanged by the alignment


def test_refusals(sv):
    state = define(sv, BOX16, [cases.one_frame(cases.cell_points(cases.distinct_cells(40)))])
    xyz, counts = cases.cell_points(cases.distinct_cells(40), 0.25)[None], np.array([40], np.int32)
    good = dict(xyz=xyz, n=None, counts=counts, poses=IDENTITY[None], origin=ZERO)
    assert sv.voxel_map_align_sums(state, **good)["sums"][0, :2].tolist() == [40, 40]
    for kw in (dict(max_dist=-0.5), dict(max_dist=np.nan), dict(max_dist=np.inf), dict(max_dist="x"), dict(poses=np.zeros((1, 3, 12))), dict(poses=np.zeros((2, 12))),
               dict(poses=np.zeros((1, 5))), dict(origin=np.zeros(3, np.int32)), dict(origin=np.zeros((2, 3), np.int32)), dict(origin=np.zeros((1, 3))),
               dict(origin=np.array([[2 ** 30 + 1, 0, 0]])), dict(xyz=np.zeros((1, 40, 2))), dict(counts=np.zeros(2, np.int32)), dict(n=np.zeros((1, 3), np.int32))):
        for f in (sv.voxel_map_align_sums, sv.voxel_map_align_sums_brute):
            with pytest.raises(ValueError):
                f(state, **dict(good, **kw))
    with pytest.raises(ValueError):
        sv.voxel_map_align_sums(state, np.zeros((65536, 1, 3)), None, np.zeros(65536, np.int32), np.zeros((65536, 12)), np.zeros((65536, 3), np.int32))
    assert sv.voxel_align_max_d2(0) == 0 and sv.voxel_align_max_d2(0.5) == 16384 and sv.voxel_align_max_d2(1) == 65536 and sv.voxel_align_max_d2(1e300) == 783363 == 3 * 511 ** 2
    loop = dict(xyz=xyz, n=None, counts=counts, poses=IDENTITY[None])
    for kw in (dict(dof=5), dict(dof=3), dict(dof=True), dict(max_dist=-1.0), dict(iterations=-1), dict(iterations=1.5), dict(eps=(1e-5,)), dict(poses=np.zeros((1, 3)))):
        with pytest.raises(ValueError):
            sv.voxel_map_align(state, **dict(loop, **kw))
    sums = sv.voxel_map_align_sums(state, **good)["sums"]
    for args in ((sums, IDENTITY[None], ZERO, state["params"], 5), (sums[:, :18], IDENTITY[None], ZERO, state["params"]), (sums, IDENTITY[None], np.zeros((1, 2), np.int32), state["params"])):
        with pytest.raises(ValueError):
            sv.voxel_align_solve(*args)
    start = shifted((0.1, 0.05, -0.1))
    kept, ok, step = sv.voxel_align_solve(sums, start[None], ZERO, state["params"], min_pairs=41)  # 40 pairs: too few
    assert np.array_equal(kept[0], start) and ok.tolist() == [False] and step.tolist() == [[0.0, 0.0]]
    res = sv.voxel_map_align(state, xyz, None, counts, start[None], min_pairs=41)
    assert np.array_equal(res["poses"][0], start) and res["ok"].tolist() == [False] and res["rounds"] == 1 and res["pairs"].tolist() == [[40]]
    over = define(sv, dict(BOX16, capacity=2), [cases.one_frame(cases.cell_points(cases.distinct_cells(3)))])
    assert over["overflowed"]
    got = _model_agrees(sv, over, (xyz, None, counts), IDENTITY[None], ZERO)
    assert not got["sums"].any() and (got["pair_key"] == -1).all() and (got["pair_d2"] == -1).all()
    res = sv.voxel_map_align(over, xyz, None, counts, start[None])
    assert np.array_equal(res["poses"][0], start) and res["ok"].tolist() == [False] and not res["sums"].any()
    empty = sv.voxel_map_align(state, np.zeros((0, 4, 3)), None, np.zeros(0, np.int32), np.zeros((0, 12)))
    assert empty["poses"].shape == (0, 12) and empty["sums"].shape == (0, 19) and empty["ok"].shape == (0,)
    origin = sv.voxel_align_origin(state["params"], np.stack([shifted((-0.3, 1e30, np.nan)), shifted((1.0, 2.5, -1e30))]))
    assert origin.tolist() == [[-77, 2 ** 30, 0], [256, 640, -2 ** 30]]  # floor, clamped, 0 for a word that is not finite
    with pytest.raises(SystemExit):
        sv.main(["-k", "nowhere", "--batch", "2", "--voxel", "0.2", "--voxel-align", "5"])  # needs --voxel-map


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z_]*voxel_align[a-z_]*)\s*\(", src))
    assert declared == {"sv_voxel_align_workspace", "sv_voxel_align_device", "sv_debug_voxel_align"}
    assert text.index("/* ---- (W)") < text.index("/* ---- (X)") < text.index("/* ---- (A)") and " *  (X) " in text
    assert set(util.pkg("engine").STAGE_SIGNATURES["voxel_align"]) == declared
    build = util.pkg("build")
    assert "voxel_align_kernels.hip" in build.SOURCES and "voxel_align.cpp" in build.SOURCES and "voxel_align_kernels.h" in build.HEADERS
    assert all(n in sv.__doc__ for n in ("voxel_map_align_sums", "voxel_align_solve", "voxel_map_align")) and "(X)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_align_kernels.hip")).read()
    assert "asm" not in source and "atomic" not in source.replace("no atomics", "")  # plain loads and stores only
    # the cell rule, the offsets, slot_of, the probe and a voxel's position are the map's own, defined once
    header = cases.check_map_table(build)
    squeezed = cases.squeeze(source)
    assert all(cases.squeeze(t) not in squeezed for t in cases.TABLE_TEXTS) and "returnvmap_key_cell(key,k)*256+(int32_t)((S/n)>>8);" in header
    assert all(source.count(call) == 1 for call in ("vmap_cell(", "vmap_offset(", "vmap_probe_goes_on(", "vmap_next_slot(", "vmap_passes(", "vmap_zq("))
    assert source.count("vmap_slot_of(") == 1 and "h + 1" not in source  # the probe's steps are the table's
    assert "wave_sum(" in source and '#include "wave_ops.h"' in source and "__shfl" not in source  # the wavefront's sums are wave_ops.h's


# ---------------------------------------------------------------------------------------------------------------- GPU

def _engine_map(eng, sv, params, calls):
    words = sv.voxel_map_params(**params)
    buf, seq = eng.voxel_map_new(words), 0
    for call in calls:
        eng.voxel_map_insert(buf, words, *[None if a is None else _cuda(a) for a in call[:4]], call[4], seq0=seq)
        seq += call[0].shape[0]
    return buf, words


def _gpu(eng, buf, words, frame, poses, origin, want_rows=True, **kw):
    xyz, n, counts = frame
    res = eng.voxel_map_align_sums(buf, words, _cuda(xyz), None if n is None else _cuda(n), _cuda(counts), poses, origin, want_rows=want_rows, **kw)
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in FIELDS}


def _agrees(eng, sv, buf, words, state, frame, poses, origin, **kw):
    """The device's dict, with and without the per-row outputs, against the definition's."""
    want = sv.voxel_map_align_sums(state, *frame, poses, origin, **kw)
    got = _gpu(eng, buf, words, frame, poses, origin, **kw)
    assert same(got, want), (kw, np.flatnonzero(got["sums"] != want["sums"]), np.flatnonzero(got["pair_key"] != want["pair_key"])[:8])
    bare = _gpu(eng, buf, words, frame, poses, origin, want_rows=False, **kw)
    assert same(bare, want, FIELDS[:1]) and bare["pair_key"] is None and bare["pair_d2"] is None, kw
    return got


@pytest.mark.gpu
def test_the_cpu_cases_on_the_device(sv, eng):
    buf, words = _engine_map(eng, sv, HAND, acases.hand_calls())
    got = _agrees(eng, sv, buf, words, define(sv, HAND, acases.hand_calls()), acases.hand_frame(), IDENTITY[None], np.array([[100, 200, -50]], np.int32))
    assert got["sums"][0, :4].tolist() == [4, 3, 6, 3 * 65536 + 2 * 8192]
    kinds, pairs = set(), 0
    for seed in range(30):
        params, calls, frame, variants, origin, max_dist, filters = acases.random_align(seed)
        buf, words = _engine_map(eng, sv, params, calls)
        state = define(sv, params, calls)
        for poses in variants:
            got = _agrees(eng, sv, buf, words, state, frame, poses, origin, max_dist=max_dist, **filters)
            pairs += int(got["sums"][:, 1].sum())
        kinds.add((str(frame[0].dtype), frame[1] is None))
        assert frame[0].shape[0] == 3 and frame[2][1] <= 0 and frame[2][2] > frame[0].shape[1]
    assert len(kinds) == 4 and pairs > 1000
    for dtype in (np.float64, np.float32):
        call = _own_pose_case(sv, dtype)
        buf, words = _engine_map(eng, sv, BOX16, [call])
        state = define(sv, BOX16, [call])
        got = _agrees(eng, sv, buf, words, state, (call[0], None, call[3]), call[4], sv.voxel_align_origin(words, call[4]))
        assert got["sums"][0, 0] == got["sums"][0, 1] == 200 - state["dropped"] and got["sums"][0, 3] == 0
    over = dict(BOX16, capacity=2)
    calls = [cases.one_frame(cases.cell_points(cases.distinct_cells(3)))]
    buf, words = _engine_map(eng, sv, over, calls)
    got = _agrees(eng, sv, buf, words, define(sv, over, calls), (calls[0][0], None, calls[0][3]), IDENTITY[None], ZERO)
    assert not got["sums"].any() and (got["pair_key"] == -1).all()


def _kernel_constants():
    text = open(os.path.join(util.pkg("build").CSRC, "voxel_align_kernels.h")).read()
    threads, rows, most = (int(re.search(r"\b%s = (\d+)," % name, text).group(1)) for name in ("VALIGN_THREADS", "VALIGN_ROWS", "VALIGN_MAX_CHUNKS"))
    assert "VALIGN_CHUNK = VALIGN_THREADS * VALIGN_ROWS," in text
    return threads, threads * rows, most


@pytest.mark.gpu
def test_row_counts(sv, eng):
    rng = np.random.default_rng(21)
    fill = [cases.one_frame(rng.uniform(0.0, 16.0, (3000, 3)), None, rng.integers(1, 9, 3000), dtype=np.float32)]
    buf, words = _engine_map(eng, sv, BOX4K, fill)
    state = define(sv, BOX4K, fill)
    assert not state["overflowed"] and len(state["key"]) > 2000
    threads, chunk, most = _kernel_constants()
    assert threads % 64 == 0 and chunk % threads == 0

    def frame_of(rows, B=1):
        cap = rows + 5 + ((rows + 5) % 64 == 0)  # never a multiple of 64
        xyz = rng.uniform(-1.0, 17.0, (B, cap, 3)).astype(np.float32 if rows % 2 else np.float64)
        return (xyz, rng.integers(-1, 9, (B, cap)).astype(np.int32), np.full(B, rows, np.int32))

    pose = lambda: shifted(rng.uniform(-0.4, 0.4, 3))  # noqa: E731
    for rows in sorted({0, 1, 63, 64, 65, threads - 1, threads, threads + 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1}):  # a lane, a wavefront, a workgroup and a chunk turn over
        frame = frame_of(rows)
        assert frame[0].shape[1] % 64 != 0
        got = _agrees(eng, sv, buf, words, state, frame, pose()[None], rng.integers(-3000, 6000, (1, 3)).astype(np.int32), max_dist=(1.0, 2.0)[rows % 2])
        assert got["sums"][0, 0] <= rows and (got["sums"][0, 1] > 0.25 * rows or rows < 16) and (got["pair_key"][0, rows:] == -1).all()
    frame = frame_of(2 * chunk + 1, B=3)  # three frames; under the hook a workgroup takes all three chunks of a frame
    frame[2][:] = (2 * chunk + 1, chunk, 7)
    poses, origin = np.stack([pose() for _ in range(3)]), rng.integers(-3000, 6000, (3, 3)).astype(np.int32)
    seen = []
    try:
        for max_chunks, skip in ((0, True), (1, True), (2, True), (0, False), (2, False)):
            assert eng.debug_voxel_align(max_chunks, skip) == 0
            seen.append(_agrees(eng, sv, buf, words, state, frame, poses, origin))
        assert all(same(s, seen[0]) for s in seen) and seen[0]["sums"][:, 1].min() > 3
        assert eng.debug_voxel_align(-1) == SV_ERR_ARG and eng.debug_voxel_align(most + 1) == SV_ERR_ARG
    finally:
        eng.debug_voxel_align(0, True)
    for b in range(3):  # every frame alone
        alone = _gpu(eng, buf, words, tuple(t[b:b + 1] for t in frame), poses[b:b + 1], origin[b:b + 1])
        assert same(alone, {k: v[b:b + 1] for k, v in seen[0].items()})
    none = _gpu(eng, buf, words, (np.zeros((0, 40, 3), np.float32), None, np.zeros(0, np.int32)), np.zeros((0, 12)), np.zeros((0, 3), np.int32))
    assert none["sums"].shape == (0, 19) and none["pair_key"].shape == (0, 40)
    no_rows = _agrees(eng, sv, buf, words, state, (np.zeros((2, 0, 3)), None, np.array([0, 5], np.int32)), np.stack([IDENTITY] * 2), np.zeros((2, 3), np.int32))
    assert not no_rows["sums"].any() and no_rows["pair_key"].shape == (2, 0)  # cap 0: no score kernel, the sums written


@pytest.mark.gpu
def test_probe_chains(sv, eng):
    import torch
    around = np.array([(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)])
    for slot in (500, 1023):  # colliding keys; from the last slot the probes wrap to slots 0 .. 6
        cells = cases.colliding_cells(sv.voxel_map_slot_of, slot, 9)
        assert (sv.voxel_map_slot_of(cells[:, 0] | (cells[:, 1] << 20) | (cells[:, 2] << 40), 1024) == slot).all()
        calls = [cases.one_frame(cases.cell_points(cells[:8]), dtype=np.float32)]  # a chain of eight; the ninth cell is not in the map
        buf, words = _engine_map(eng, sv, PROBE_BOX, calls)
        state = define(sv, PROBE_BOX, calls)
        before = buf.clone()
        own = (cases.cell_points(cells, 0.25)[None], None, np.array([9], np.int32))
        got = _agrees(eng, sv, buf, words, state, own, IDENTITY[None], ZERO)
        assert got["pair_key"][0, :8].tolist() == [key_of(c) for c in cells[:8]] and (got["pair_d2"][0, :8] == 3 * 64 ** 2).all()  # each through its chain
        near = (cells[:8, None, :] + around[None]).reshape(-1, 3)
        near = near[((near >= 0) & (near < 64)).all(1)]
        rows = (cases.cell_points(near, 0.6)[None], None, np.array([len(near)], np.int32))  # from every cell around a chain's voxel
        got = _agrees(eng, sv, buf, words, state, rows, IDENTITY[None], ZERO, max_dist=2.0)
        assert (got["pair_key"] >= 0).all() and got["sums"][0, 1] == len(near)
        torch.cuda.synchronize()
        assert torch.equal(buf, before)  # the map is only read
    cells = cases.distinct_cells(64 ** 3, 64)
    full = cells[(cells[:, 0] >= 3) & (cells[:, 0] <= 60)][::97][:512]  # a table as full as its capacity allows, nothing within two cells of the faces x = 0 and x = 63
    calls = [cases.one_frame(cases.cell_points(full), dtype=np.float32)]
    buf, words = _engine_map(eng, sv, PROBE_BOX, calls)
    state = define(sv, PROBE_BOX, calls)
    assert len(state["key"]) == 512 and not state["overflowed"]
    outer = np.array([(0, 0, 0), (0, 63, 0), (0, 30, 63), (63, 63, 63), (63, 0, 5), (1, 1, 1), (62, 20, 20)])
    got = _agrees(eng, sv, buf, words, state, (cases.cell_points(outer, 0.1)[None], None, np.array([len(outer)], np.int32)), IDENTITY[None], ZERO, max_dist=2.0)
    assert (got["pair_key"] == -1).all() and got["sums"][0].tolist() == [len(outer)] + [0] * 18  # no cell outside the box is "found"
    inner = full[::5] + np.array([1, 0, 0])
    got = _agrees(eng, sv, buf, words, state, (cases.cell_points(inner, 0.3)[None], None, np.array([len(inner)], np.int32)), IDENTITY[None], ZERO, max_dist=2.0)
    assert (got["pair_key"] >= 0).all()


@pytest.mark.gpu
def test_edges_and_tombstones_on_the_device(sv, eng):
    params, calls, frame = acases.edge_case()
    buf, words = _engine_map(eng, sv, params, calls)
    state = define(sv, params, calls)
    for max_dist in (1.0, 2.0):
        got = _agrees(eng, sv, buf, words, state, frame, IDENTITY[None], np.array([[2048, 2048, 2048]], np.int32), max_dist=max_dist)
        assert (got["pair_key"] >= 0).all()
    far = [cases.one_frame(cases.cell_points([(8, 8, 8)]))]
    buf, words = _engine_map(eng, sv, BOX16, far)
    corner = (np.array([[[0.5, 0.5, 0.5], [15.5, 15.5, 15.5], [0.5, 15.5, 0.5]]]), None, np.array([3], np.int32))
    got = _agrees(eng, sv, buf, words, define(sv, BOX16, far), corner, IDENTITY[None], ZERO, max_dist=2.0)
    assert (got["pair_key"] == -1).all() and got["sums"][0].tolist() == [3] + [0] * 18
    params, calls, frame = acases.long_case()
    buf, words = _engine_map(eng, sv, params, calls)
    got = _agrees(eng, sv, buf, words, define(sv, params, calls), frame, IDENTITY[None], np.array([[2 ** 28 - 512, 0, 0]], np.int32), max_dist=2.0)
    assert got["pair_key"].tolist() == [[key_of((2 ** 20 - 2, 0, 0))] * 3 + [key_of((0, 1, 0))]]
    params, calls, carve, frame = acases.tombstone_case()
    for also in (False, True):
        buf, words = _engine_map(eng, sv, params, calls)
        state = define(sv, params, calls)
        sv.voxel_map_carve(state, **carve, apply=True)
        res = eng.voxel_map_carve(buf, words, _cuda(carve["xyz"]), None, _cuda(carve["counts"]), carve["poses"], origin=carve["origin"], seq0=1, apply=True)
        if also:
            args = (np.array([[[6.5, 9.5, 5.5]]]), None, carve["counts"], carve["poses"])
            sv.voxel_map_carve(state, *args, origin=(6.5, 2.5, 5.5), seq0=1, apply=True)
            res = eng.voxel_map_carve(buf, words, _cuda(args[0]), None, _cuda(args[2]), args[3], origin=(6.5, 2.5, 5.5), seq0=1, apply=True)
        assert int(res.stats.cpu().numpy()[3]) == 1 and state["n"].tolist() == [0, 0 if also else 1]
        for kw in (dict(min_n=1), dict(min_n=0), dict(min_n=0, min_rows=0, since=-5), dict(min_n=-3, min_rows=-3, since=-2 ** 31)):
            got = _agrees(eng, sv, buf, words, state, frame, IDENTITY[None], ZERO, **kw)
            assert got["pair_key"].tolist() == [[-1 if also else key_of((6, 5, 5))]]


@pytest.mark.gpu
def test_sums_of_64_bits(sv, eng):
    rng = np.random.default_rng(9)
    fill = [cases.one_frame(rng.uniform(0.0, 16.0, (600, 3)))]
    buf, words = _engine_map(eng, sv, BOX4K, fill)
    state = define(sv, BOX4K, fill)
    xyz = rng.uniform(0.5, 15.5, (1, 3, 3))
    frame = (xyz, np.array([[2 ** 20 - 1, 2 ** 20 - 3, 2 ** 19 + 7]], np.int32), np.array([3], np.int32))
    origin = np.array([[-2 ** 20, 2 ** 20 - 7, -2 ** 20 + 3]], np.int32)  # r about 2^20: w r^2 about 2^60 a row
    want = sv.voxel_map_align_sums_brute(state, *frame, IDENTITY[None], origin, max_dist=2.0)
    assert want["sums"][0, 1] == 3 and 2 ** 60 < int(np.abs(want["sums"]).max()) < 2 ** 62  # the definition itself is far from wrapping
    assert int(np.abs(want["sums"][0, 4:10]).max()) > 2 ** 40  # and already P and Q need more than 32 bits
    got = _agrees(eng, sv, buf, words, state, frame, IDENTITY[None], origin, max_dist=2.0)
    assert same(got, want)
    heavy = (xyz, np.full((1, 3), 2 ** 31 - 1, np.int32), frame[2])  # the largest weight, about an origin at the rows
    got = _agrees(eng, sv, buf, words, state, heavy, IDENTITY[None], np.array([[2048, 2048, 2048]], np.int32), max_dist=2.0)
    assert got["sums"][0, 2] == 3 * (2 ** 31 - 1) and same(got, sv.voxel_map_align_sums_brute(state, *heavy, IDENTITY[None], np.array([[2048, 2048, 2048]], np.int32), max_dist=2.0))


@pytest.mark.gpu
def test_the_loop_on_the_device(sv, eng):
    rigmod = util.pkg("rig")
    truth = acases.scene_truth(sv)
    for dtype, dof, which in ((np.float64, 6, "all"), (np.float32, 6, "all"), (np.float64, 4, "yaw")):
        call, (xyz, n, counts) = acases.scene_case(dtype)
        worlds = [rigmod.VoxelMap(device=d, **mcases.SCENE_BOX) for d in ("cuda", "cpu")]
        worlds[0].update(*[None if a is None else _cuda(a) for a in call[:4]], call[4])
        worlds[1].update(*call)
        start = acases.scene_start(sv, *acases.SCENE_STARTS[which])[None]
        want = sv.voxel_map_align(worlds[1]._state, xyz, n, counts, start, iterations=15, dof=dof)
        res = eng.voxel_map_align(worlds[0].buffer, worlds[0].params, _cuda(xyz), None, _cuda(counts), start, iterations=15, dof=dof)
        assert isinstance(res, eng.VoxelAlignResult) and res.sums.is_cuda and res.poses.dtype == np.float64
        for k in ("poses", "ok", "pairs", "rms"):
            assert np.array_equal(getattr(res, k), want[k]) and getattr(res, k).dtype == want[k].dtype, k  # equal, not close: the fit is shared and the sums are equal
        assert res.rounds == want["rounds"] and np.array_equal(res.sums.cpu().numpy(), want["sums"])
        (poses, got), (poses_cpu, got_cpu) = (w.align(x, None, c, p, iterations=15, dof=dof) for w, x, c, p in
                                              ((worlds[0], _cuda(xyz), _cuda(counts), _cuda(start)), (worlds[1], xyz, counts, start)))
        assert np.array_equal(poses, poses_cpu) and np.array_equal(poses, want["poses"]) and got.rounds == got_cpu.rounds == want["rounds"]
        assert np.array_equal(got.rms, got_cpu.rms) and np.array_equal(got.pairs, got_cpu.pairs) and got.ok.tolist() == got_cpu.ok.tolist() == [True]
        rot0, tr0 = acases.pose_error(start[0], truth)
        rot, tr = acases.pose_error(poses[0], truth)
        assert rot < rot0 / 10 and tr < tr0 / 10 and got.pairs[-1, 0] == 600
        assert worlds[0].stats() == {"claimed": 978, "dropped": 0, "overflowed": False} and worlds[0].seq == 1
    for kw in (dict(max_dist=-1.0), dict(dof=5), dict(poses=np.zeros((2, 12))), dict(xyz=_cuda(xyz).cpu())):
        with pytest.raises(ValueError):
            eng.voxel_map_align(worlds[0].buffer, worlds[0].params, **dict(dict(xyz=_cuda(xyz), n=None, counts=_cuda(counts), poses=start), **kw))
    for kw in (dict(origin=np.zeros((2, 3), np.int32)), dict(origin=np.zeros((1, 3))), dict(origin=_cuda(np.zeros((1, 3), np.int64))), dict(max_dist=np.nan),
               dict(poses=np.zeros((1, 3, 12))), dict(counts=_cuda(counts).long()), dict(min_n=0.5), dict(since=2 ** 31)):
        with pytest.raises(ValueError):
            eng.voxel_map_align_sums(worlds[0].buffer, worlds[0].params, **dict(dict(xyz=_cuda(xyz), n=None, counts=_cuda(counts), poses=start, origin=ZERO), **kw))
    with pytest.raises(ValueError):
        big = _cuda(np.zeros((65536, 1, 3), np.float32))
        eng.voxel_map_align_sums(worlds[0].buffer, worlds[0].params, big, None, _cuda(np.zeros(65536, np.int32)), np.zeros((65536, 12)), np.zeros((65536, 3), np.int32))
    params = dict(BOX16, capacity=2)
    calls = [cases.one_frame(cases.cell_points(cases.distinct_cells(3)))]
    over = rigmod.VoxelMap(device="cuda", **params)
    over.update(*[None if a is None else _cuda(a) for a in calls[0][:4]], calls[0][4])
    start = shifted((0.1, 0.0, 0.0))[None]
    poses, res = over.align(_cuda(calls[0][0]), None, _cuda(calls[0][3]), start)
    assert np.array_equal(poses, start) and res.ok.tolist() == [False] and res.rounds == 1 and not res.sums.any().item()


@pytest.mark.gpu
def test_the_c_entry_refuses(sv, eng):
    import ctypes
    import torch
    words = sv.voxel_map_params(**BOX16)
    buf, _ = _engine_map(eng, sv, BOX16, [cases.one_frame(cases.cell_points(cases.distinct_cells(40)), dtype=np.float32)])
    before = buf.clone()
    xyz, n, counts = _cuda(cases.cell_points(cases.distinct_cells(40)).astype(np.float32)[None]), _cuda(np.full((1, 40), 2, np.int32)), _cuda(np.array([40], np.int32))
    poses, origin = _cuda(IDENTITY[None]), _cuda(ZERO)
    L = eng.voxel_align_lib()
    spec, nbytes, st = eng.voxel_map_spec(words), buf.numel() * 8, torch.cuda.current_stream().cuda_stream
    _, chunk, most = _kernel_constants()
    need = ctypes.c_size_t(7)
    for cap, B in ((-1, 1), (40, -1), (40, 65536)):
        assert L.sv_voxel_align_workspace(cap, B, ctypes.byref(need)) == SV_ERR_ARG and need.value == 7 and b"sv_voxel_align" in L.sv_last_error(None)
    assert L.sv_voxel_align_workspace(40, 1, None) == SV_ERR_ARG
    assert L.sv_voxel_align_workspace(0, 0, ctypes.byref(need)) == 0 and need.value == 0
    assert L.sv_voxel_align_workspace(chunk + 1, 3, ctypes.byref(need)) == 0 and need.value == 3 * 2 * 19 * 8
    assert L.sv_voxel_align_workspace(2 ** 31 - 1, 2, ctypes.byref(need)) == 0 and need.value == 2 * most * 19 * 8  # at most so many chunks
    assert L.sv_voxel_align_workspace(40, 1, ctypes.byref(need)) == 0 and need.value == 19 * 8  # one chunk
    ws = torch.full((need.value // 8 + 2,), 77, dtype=torch.int64, device="cuda")
    shapes = (("sums", (1, 19), torch.int64), ("pair_key", (1, 40), torch.int64), ("pair_d2", (1, 40), torch.int32))
    out = {k: torch.full(shape, 77, dtype=dt, device="cuda") for k, shape, dt in shapes}

    def spec_with(**kw):
        s = eng.voxel_map_spec(words)
        for k, v in kw.items():
            if k in ("lo", "hi", "reserved"):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return ctypes.byref(s)

    good = [buf.data_ptr(), nbytes, ctypes.byref(spec), xyz.data_ptr(), 0, n.data_ptr(), counts.data_ptr(), poses.data_ptr(), origin.data_ptr(), 1, 40, 65536, 1, 1, 0] + \
        [out[k].data_ptr() for k, _, _ in shapes] + [ws.data_ptr(), need.value, st]
    bad = {0: [None, buf.data_ptr() + 8], 1: [nbytes - 8, 0],
           2: [None, spec_with(size=0.0), spec_with(size=float("nan")), spec_with(capacity=0), spec_with(capacity=2 ** 26 + 1), spec_with(reserved=(3, 1)),
               spec_with(hi=(1, 0.0)), spec_with(lo=(2, float("-inf"))), spec_with(size=1e-6)],
           3: [None, xyz.data_ptr() + 2], 4: [2, -1], 5: [n.data_ptr() + 2], 6: [None, counts.data_ptr() + 1], 7: [None, poses.data_ptr() + 4],
           8: [None, origin.data_ptr() + 2], 9: [-1, 65536], 10: [-1], 11: [-1, 783364, 2 ** 31 - 1], 15: [None, out["sums"].data_ptr() + 4],
           16: [None, out["pair_key"].data_ptr() + 4], 17: [None, out["pair_d2"].data_ptr() + 2], 18: [None, ws.data_ptr() + 4], 19: [need.value - 1, 0]}
    for at, values in bad.items():
        for v in values:
            assert L.sv_voxel_align_device(*(good[:at] + [v] + good[at + 1:])) == SV_ERR_ARG and b"sv_voxel_align" in L.sv_last_error(None), (at, v)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and all((t == 77).all().item() for t in out.values()) and (ws == 77).all().item()  # nothing was enqueued
    assert L.sv_voxel_align_device(*(good[:3] + [None, 0, None, None, None, None, 0, 40, 65536, 1, 1, 0] + [None] * 3 + [None, 0, st])) == 0  # an empty batch needs no pointer
    torch.cuda.synchronize()
    assert all((t == 77).all().item() for t in out.values()) and (ws == 77).all().item()  # batch 0 touches nothing
    assert L.sv_voxel_align_device(*(good[:16] + [None, None] + good[18:])) == 0  # only the sums
    torch.cuda.synchronize()
    assert out["sums"][0, :4].tolist() == [40, 40, 80, 0] and all((out[k] == 77).all().item() for k in FIELDS[1:]) and (ws[-2:] == 77).all().item()
    assert L.sv_voxel_align_device(*(good[:11] + [783363] + good[12:])) == 0 and L.sv_voxel_align_device(*good) == 0  # and the good calls go through
    torch.cuda.synchronize()
    assert out["pair_key"][0].tolist() == [key_of(c) for c in cases.distinct_cells(40)] and not out["pair_d2"].any().item() and torch.equal(buf, before)


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
    base = ["-k", str(tmp_path / "kitti"), "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt")]
    alone, both = (str(tmp_path / name) for name in ("alone.ply", "both.ply"))
    sv.main(base + ["--batch", "1", "--voxel-map", alone, "--voxel-align", "3,1.5,4"])  # frame 1 against frame 0
    sv.main(base + ["--batch", "2", "--voxel-map", both, "--voxel-match", "0.2,0,0,0,3,1,1,1", "--voxel-align", "2"])
    for stem, dof in ((alone, 4), (both, 6)):
        lines = [[float(w) for w in line.split()] for line in open(os.path.splitext(stem)[0] + ".aligned.txt")]
        assert len(lines) == 2 and all(len(words) == 12 and np.isfinite(words).all() for words in lines)
        assert lines[0] == sv.voxel_map_pose(0.0, 0.0, 0.0).tolist()  # frame 0 goes in where its line says
        R = np.array(lines[1][:9]).reshape(3, 3)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-9 and np.abs(np.array(lines[1][9:]) - (0.8, 0.05, 0.0)).max() < 1.0
        assert dof == 6 or lines[1][6:9] == [0.0, 0.0, 1.0]
        assert os.path.getsize(stem) > 1000
    assert len(open(os.path.splitext(both)[0] + ".poses.txt").read().split()) == 8 and not os.path.exists(os.path.splitext(alone)[0] + ".poses.txt")
    for bad in ("0", "3,-1", "3,1,5", "3,1,6,1", "x"):
        with pytest.raises(SystemExit):
            sv.main(base + ["--batch", "1", "--voxel-map", alone, "--voxel-align", bad])
    with pytest.raises(SystemExit):
        sv.main(base + ["--batch", "1", "--voxel-align", "3"])
