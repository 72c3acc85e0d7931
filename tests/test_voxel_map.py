"""The world-fixed voxel map (group (Q)): stereo_vision.sv.voxel_map_insert / voxel_map_rows against the per-row model of
voxel_map_cases, and engine.voxel_map_* / rig.VoxelMap / the CLI against the definition.  Every comparison is shape, dtype and bits."""
import math
import os

import numpy as np
import pytest

import util
import voxel_map_cases as cases
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_map_cases import BOX16, FIELDS, IDENTITY, PROBE_BOX, QUARTER

SV_ERR_ARG = -1


def _same(got, want, fields=FIELDS):
    for k in fields:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            return False
    return got["count"] == want["count"]


def _define(sv, params, calls):
    state, seq = sv.voxel_map_state(sv.voxel_map_params(**params)), 0
    for call in calls:
        sv.voxel_map_insert(state, *call, seq0=seq)
        seq += call[0].shape[0]
    return state


def _dev(call):
    return tuple(None if a is None else _cuda(a) for a in call)


def _host(rows):
    return {k: v if k == "count" else v.cpu().numpy() for k, v in rows.items()}


def _engine_map(eng, sv, params, calls):
    words = sv.voxel_map_params(**params)
    buf, seq = eng.voxel_map_new(words), 0
    for call in calls:
        eng.voxel_map_insert(buf, words, *_dev(call[:4]), call[4], seq0=seq)
        seq += call[0].shape[0]
    return buf, words


def _engine_rows(eng, sv, params, calls, **kw):
    buf, words = _engine_map(eng, sv, params, calls)
    return _host(eng.voxel_map_rows(buf, words, **kw)), eng.voxel_map_stats(buf)


def _rig_map(params, calls, device="cuda"):
    world = util.pkg("rig").VoxelMap(params["lo"], params["hi"], params["size"], params["capacity"], device=device)
    for call in calls:
        world.update(*(_dev(call[:4]) if device == "cuda" else call[:4]), call[4])
    return world


# ---------------------------------------------------------------------------------------------------------------- CPU

HAND = dict(lo=(0.0, 0.0, -0.9), hi=(4.0, 4.0, 1.1), size=1.0, capacity=512)  # 4 x 4 x 2 cells


def _hand_calls():
    top = math.nextafter(1.1, 0.0)  # hi minus one ulp: (top - lo) / size rounds to 2.0, so the cell is clamped to 1 and u to 65535
    assert (top - 0.5) + 0.5 == top and top - (-0.9) == 2.0
    f0 = np.array([[2.0, -1.5, -0.4], [np.nan, 1.0, 0.0], [1.0, 0.0, -0.4]])  # a quarter turn: Pw = (-y, x, z); (1.5, 2.0, -0.4) lies on a
    f1 = np.array([[0.5, 2.25, top - 0.5], [0.5, 2.0, -0.9], [9.0, 9.0, 9.0]])  # cell boundary in y; NaN; (0, 1, -0.4) lies at lo in x
    xyz = np.stack([f0, f1])
    color = np.array([[[10, 20, 30, 40]] * 3, [[1, 2, 3, 4], [110, 120, 130, 140], [0, 0, 0, 0]]], np.uint8)
    n = np.array([[3, 1, 1], [5, 2, 1]], np.int32)
    shift = IDENTITY.copy()
    shift[9:] = (1.0, 0.0, 0.5)
    return [(xyz, color, n, np.array([3, 2], np.int32), np.stack([QUARTER, shift]))]  # frame 1 contributes two rows: five rows in all


def test_hand_case(sv):
    state = _define(sv, HAND, _hand_calls())
    got = sv.voxel_map_rows(state, dtype="f64")
    assert state["dropped"] == 2 and not state["overflowed"] and got["count"] == 2
    a, b = 1 | 2 << 20, 1 | 2 << 20 | 1 << 40
    assert got["key"].tolist() == [a, b] and got["cell"].tolist() == [[1, 2, 0], [1, 2, 1]] and got["cell"].dtype == np.int32
    assert got["n"].tolist() == [5, 5] and got["m"].tolist() == [2, 1] and got["n"].dtype == got["m"].dtype == np.int64
    assert got["first_seq"].tolist() == [0, 1] and got["last_seq"].tolist() == [1, 1] and got["first_seq"].dtype == np.int32
    assert state["S"].tolist() == [[5 * 32768, 0, 5 * 32768], [5 * 32768, 5 * 16384, 5 * 65535]]
    assert state["C"].tolist() == [[250, 300, 350, 400], [5, 10, 15, 20]]
    assert got["color"].tolist() == [[50, 60, 70, 80], [1, 2, 3, 4]] and got["color"].dtype == np.uint8
    want = [[1 + (163840 + 2.5) / 327680, 2 + 2.5 / 327680, -0.9 + (0 + (163840 + 2.5) / 327680) * 1.0],
            [1 + (163840 + 2.5) / 327680, 2 + (81920 + 2.5) / 327680, -0.9 + (1 + (327675 + 2.5) / 327680) * 1.0]]
    assert got["xyz"].tolist() == want and got["xyz"].dtype == np.float64
    assert _same(got, cases.model_voxel_map(HAND, _hand_calls(), dtype="f64"))
    f32 = sv.voxel_map_rows(state)
    assert f32["xyz"].dtype == np.float32 and np.array_equal(f32["xyz"], got["xyz"].astype(np.float32))
    cpu = _rig_map(HAND, _hand_calls(), device="cpu")  # rig.VoxelMap on CPU tensors runs the definition
    assert _same(_host(cpu.rows(dtype="f64")), got) and cpu.stats() == {"claimed": 2, "dropped": 2, "overflowed": False} and cpu.seq == 2
    cpu.reset()
    assert cpu.seq == 0 and cpu.rows()["count"] == 0 and cpu.stats() == {"claimed": 0, "dropped": 0, "overflowed": False}


def test_definition_against_model(sv):
    todo = [cases.random_case(s) for s in range(50)] + [(p, c) for p, c, _ in cases.painted_cases().values()]
    kinds = set()
    for params, calls in todo:
        state = _define(sv, params, calls)
        for dtype in ("f32", "f64"):
            want = cases.model_voxel_map(params, calls, dtype=dtype)
            assert _same(sv.voxel_map_rows(state, dtype=dtype), want)
        assert state["dropped"] == want["dropped"] and len(state["key"]) == want["claimed"]
        kinds.add((str(calls[0][0].dtype), calls[0][1] is None, calls[0][2] is None))
    assert len(kinds) >= 8  # f32 and f64, with and without colours, with and without weights


def test_painted_cases_are_their_layouts(sv):
    painted = cases.painted_cases()
    for name, (params, calls, updates) in painted.items():
        if updates is not None:
            assert cases.table_updates(params, calls) == updates, name
    keys = cases.frame_keys(BOX16, painted["one_voxel_257"][1][0])[0]
    assert len(keys) == 257 and len(set(keys)) == 1 and keys[0] is not None
    keys = cases.frame_keys(BOX16, painted["every_row_its_own"][1][0])[0]
    assert len(set(keys)) == 300 and cases.table_updates(BOX16, painted["every_row_its_own"][1], combine=False) == 300
    keys = cases.frame_keys(BOX16, painted["run_cut_by_a_dropped_row"][1][0])[0]
    assert keys[17] is None and len(set(keys)) == 2
    big = sv.voxel_map_rows(_define(sv, BOX16, painted["largest_payload"][1]))
    assert big["n"].tolist() == [64 * (2 ** 31 - 1)] and big["color"].tolist() == [[255] * 4] and big["cell"].tolist() == [[15, 15, 15]]
    assert _define(sv, BOX16, painted["largest_payload"][1])["S"].tolist() == [[64 * (2 ** 31 - 1) * 65535] * 3]  # > 2^52: the 64-bit carries
    assert 1 < cases.table_updates(BOX16, painted["short_runs"][1]) < len(painted["short_runs"][1][0][0][0])


def test_probe_layouts(sv):
    for slot in (500, 1023):
        c = cases.colliding_cells(sv.voxel_map_slot_of, slot, 8)
        key = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
        assert len(set(key.tolist())) == 8 and (sv.voxel_map_slot_of(key, 1024) == slot).all()  # slot 1023: the probes wrap to slots 0 .. 6
    assert sv.voxel_map_slots(512) == 1024


def test_order_freedom(sv):
    rng = np.random.default_rng(3)
    B, cap = 4, 60
    xyz = rng.uniform(-0.5, 4.5, (B, cap, 3)).astype(np.float32)
    color, n = rng.integers(0, 256, (B, cap, 4)).astype(np.uint8), rng.integers(0, 9, (B, cap)).astype(np.int32)
    counts = np.full(B, cap, np.int32)
    poses = sv.voxel_map_pose(rng.uniform(0, 1, B), rng.uniform(0, 1, B), rng.uniform(-0.3, 0.3, B), 0.5)
    params = dict(lo=(0.0, 0.0, 0.0), hi=(4.0, 4.0, 4.0), size=1.0, capacity=512)
    want = sv.voxel_map_rows(_define(sv, params, [(xyz, color, n, counts, poses)]))
    assert want["count"] > 40 and (want["first_seq"] != want["last_seq"]).any()
    perm_f, perm_r = rng.permutation(B), rng.permutation(cap)
    shuffled = (xyz[perm_f][:, perm_r], color[perm_f][:, perm_r], n[perm_f][:, perm_r], counts, poses[perm_f])
    got = sv.voxel_map_rows(_define(sv, params, [shuffled]))
    assert _same(got, want, [f for f in FIELDS if not f.endswith("_seq")])
    # the sequence numbers follow the numbering: frame perm_f[j] is now frame j
    inverse = np.argsort(perm_f)
    renumbered = _define(sv, params, [(xyz[b:b + 1], color[b:b + 1], n[b:b + 1], counts[b:b + 1], poses[b:b + 1]) for b in range(B)])
    assert _same(sv.voxel_map_rows(renumbered), want)  # one update of B frames = B updates of one frame
    per_frame = [sv.voxel_map_rows(_define(sv, params, [(xyz[b:b + 1], color[b:b + 1], n[b:b + 1], counts[b:b + 1], poses[b:b + 1])]))["key"] for b in range(B)]
    first = {int(k): min(int(inverse[b]) for b in range(B) if k in per_frame[b]) for k in want["key"]}
    assert got["first_seq"].tolist() == [first[int(k)] for k in got["key"]]


def test_filters(sv):
    pts = cases.cell_points(np.repeat(cases.distinct_cells(6), [1, 2, 3, 4, 5, 6], 0))
    w = np.full(len(pts), 2, np.int32)
    calls = [cases.one_frame(pts, None, w), cases.one_frame(pts[:6], None, w[:6]), cases.one_frame(pts[:3], None, w[:3])]  # seq 0, 1, 2
    state = _define(sv, BOX16, calls)
    full = sv.voxel_map_rows(state)
    assert full["n"].tolist() == [6, 12, 12, 8, 10, 12] and full["m"].tolist() == [3, 6, 6, 4, 5, 6] and full["last_seq"].tolist() == [2, 2, 1, 0, 0, 0]
    for kw, keep in ((dict(min_n=9), full["n"] >= 9), (dict(min_n=10), full["n"] >= 10), (dict(min_n=11), full["n"] >= 11),
                     (dict(min_rows=4), full["m"] >= 4), (dict(min_rows=5), full["m"] >= 5), (dict(min_rows=6), full["m"] >= 6),
                     (dict(since=0), full["last_seq"] >= 0), (dict(since=1), full["last_seq"] >= 1), (dict(since=2), full["last_seq"] >= 2),
                     (dict(since=3), full["last_seq"] >= 3), (dict(min_n=10, min_rows=5, since=1), (full["n"] >= 10) & (full["last_seq"] >= 1))):
        got = sv.voxel_map_rows(state, **kw)
        assert got["count"] == int(keep.sum()) and _same(got, dict({f: full[f][keep] for f in FIELDS}, count=int(keep.sum()))), kw
        assert _same(got, cases.model_voxel_map(BOX16, calls, **kw))


def test_the_hash(sv, eng):
    rng = np.random.default_rng(11)
    keys = np.concatenate([rng.integers(0, 2 ** 60, 10000), [0, 1, 2 ** 20 - 1, 2 ** 20, 2 ** 40, 2 ** 60 - 1, (2 ** 20 - 1) << 40, -1]]).astype(np.int64)
    L = eng.voxel_map_lib()
    for slots in (1024, 2 ** 27):
        want = sv.voxel_map_slot_of(keys, slots)
        assert want.dtype == np.int64 and want.min() >= 0 and want.max() < slots
        assert [L.sv_voxel_map_slot_of(int(k), slots) for k in keys] == want.tolist()
    assert eng.voxel_map_slot_of(5, 2) == int(sv.voxel_map_slot_of(5, 2)) and L.sv_voxel_map_slot_of(5, 1000) == -1 and L.sv_voxel_map_slot_of(5, 1) == -1
    for bad in (0, 1, 1000, 2 ** 33, 1024.5, True):
        with pytest.raises(ValueError):
            sv.voxel_map_slot_of(keys, bad)
    for capacity, slots in ((1, 1024), (512, 1024), (513, 2048), (2 ** 26, 2 ** 27)):
        assert sv.voxel_map_slots(capacity) == slots == L.sv_voxel_map_slots(capacity)
        assert L.sv_voxel_map_bytes(capacity) == 32 + slots * 88 + slots // 256 * 4
    assert L.sv_voxel_map_slots(0) == -1 and L.sv_voxel_map_slots(2 ** 26 + 1) == -1 and L.sv_voxel_map_bytes(0) == 2 ** 64 - 1


def test_params_and_pose(sv):
    ok = sv.voxel_map_params((0, 0, 0), (1048576 * 0.5, 1, 1), 0.5, 2 ** 26)  # 2^20 cells, the largest capacity
    assert ok["cells"] == (2 ** 20, 2, 2) and ok["capacity"] == 2 ** 26 and ok["lo"] == (0.0, 0.0, 0.0)
    assert sv.voxel_map_params((0, 0, 0), (1, 1, 1), 4.0, 1)["cells"] == (1, 1, 1)
    inf = float("inf")
    for lo, hi, size, capacity in (((0, 0, 0), (1048577 * 0.5, 1, 1), 0.5, 10), ((0, 0, 0), (1, 1, 1), 1.0, 0), ((0, 0, 0), (1, 1, 1), 1.0, 2 ** 26 + 1),
                                   ((0, 0, 0), (1, 1, 1), 0.0, 10), ((0, 0, 0), (1, 1, 1), -1.0, 10), ((0, 0, 0), (1, 1, 1), inf, 10),
                                   ((0, 0, 0), (1, 0, 1), 1.0, 10), ((0, 0, 1), (1, 1, 1), 1.0, 10), ((0, -inf, 0), (1, 1, 1), 1.0, 10),
                                   ((0, 0, 0), (1, 1, float("nan")), 1.0, 10), ((0, 0, 0), (1, 1, 1), 1.0, 2.5), ((0, 0, 0), (1, 1, 1), 1.0, None),
                                   (None, (1, 1, 1), 1.0, 10)):
        with pytest.raises(ValueError):
            sv.voxel_map_params(lo, hi, size, capacity)
    yaw = np.array([0.0, 0.3, np.pi / 2, -2.0])
    p, q = sv.voxel_map_pose([1, 2, 3, 4], [5, 6, 7, 8], yaw, 0.25), sv.occupancy_pose([1, 2, 3, 4], [5, 6, 7, 8], yaw)
    assert p.shape == (4, 12) and p.dtype == np.float64
    assert np.array_equal(p[:, [9, 10, 0, 3]], q) and np.array_equal(p[:, 1], -q[:, 3]) and np.array_equal(p[:, 4], q[:, 2])
    assert (p[:, [2, 5, 6, 7]] == 0).all() and (p[:, 8] == 1).all() and (p[:, 11] == 0.25).all()
    assert sv.voxel_map_pose(1.0, 2.0, 0.0).tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 2, 0]
    assert np.array_equal(sv.voxel_map_pose_words(q), sv.voxel_map_pose([1, 2, 3, 4], [5, 6, 7, 8], yaw)) and sv.voxel_map_pose_words(p) is not None
    with pytest.raises(ValueError):
        sv.voxel_map_pose_words(np.zeros((2, 3)))
    state = sv.voxel_map_state(BOX16)
    one = cases.one_frame(cases.cell_points([(1, 1, 1)]))
    for seq0 in (-1, 2 ** 31 - 1, 0.5):
        with pytest.raises(ValueError):
            sv.voxel_map_insert(state, *one, seq0=seq0)
    sv.voxel_map_insert(state, *one, seq0=2 ** 31 - 2)
    assert sv.voxel_map_rows(state)["last_seq"].tolist() == [2 ** 31 - 2]
    # a map that ever held more than its capacity reports -1 and no rows
    small = sv.voxel_map_state(dict(BOX16, capacity=2))
    sv.voxel_map_insert(small, *cases.one_frame(cases.cell_points(cases.distinct_cells(2))))
    assert sv.voxel_map_rows(small)["count"] == 2
    sv.voxel_map_insert(small, *cases.one_frame(cases.cell_points(cases.distinct_cells(3))))
    over = sv.voxel_map_rows(small)
    assert over["count"] == -1 and all(len(over[f]) == 0 for f in FIELDS) and over["xyz"].shape == (0, 3)


def test_header_build_and_loader_agree(sv, eng):
    import re
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z_]*voxel_map[a-z_]*)\s*\(", src))
    assert declared == {"sv_voxel_map_slots", "sv_voxel_map_bytes", "sv_voxel_map_slot_of", "sv_voxel_map_clear_device", "sv_voxel_map_insert_device",
                        "sv_voxel_map_rows_device", "sv_debug_voxel_map"}
    assert text.index("/* ---- (P)") < text.index("/* ---- (Q)") < text.index("/* ---- (A)") and " *  (Q) " in text
    L = eng.voxel_map_lib()
    assert all(hasattr(L, n) for n in declared) and set(eng.STAGE_SIGNATURES["voxel_map"]) == declared
    build = util.pkg("build")
    assert "voxel_map_kernels.hip" in build.SOURCES and "voxel_map.cpp" in build.SOURCES and "voxel_map_kernels.h" in build.HEADERS
    assert all(n in sv.__doc__ for n in ("voxel_map_params", "voxel_map_pose", "voxel_map_insert", "voxel_map_rows", "voxel_map_slot_of")) and "(Q)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_map_kernels.hip")).read()
    assert "asm" not in source and "atomicAdd(float" not in source
    header = cases.check_map_table(build)
    assert "sv::vmap_slot_of(" in open(os.path.join(build.CSRC, "voxel_map.cpp")).read()  # test_the_hash covers the function the kernels inline
    # the insert keeps the claiming probe around its update, restated from the header's vmap_claim: the same text in both files
    for line in ("const uint32_t last = (uint32_t)(((size_t)1 << log2_slots) - 1);", "uint32_t h = vmap_slot_of(log2_slots, key)", cases.PROBE_LOOP,
                 "if ((probe & 15) == 15 && vmap_overflowed_meanwhile(head)) break;", "unsigned long long *e = table + (size_t)h * VMAP_ENTRY_WORDS;",
                 "const unsigned long long old = atomicCAS(e + VMAP_KEY, VMAP_EMPTY, key);", "if (old != VMAP_EMPTY && old != key) continue;", "atomicOr(head + 1, 1u);"):
        assert cases.squeeze(line) in cases.squeeze(source) and cases.squeeze(line) in header, line


def test_cli_argument_errors(sv, tmp_path):
    poses, ply, out = str(tmp_path / "poses.txt"), str(tmp_path / "ply"), str(tmp_path / "drive.ply")
    with open(poses, "w") as f:
        f.write("0 0 0\n")
    full = ["--batch", "2", "--ply", ply, "--voxel", "0.2", "--poses", poses, "--voxel-map", out]
    for leave in ("--batch", "--ply", "--voxel", "--poses"):
        at = full.index(leave)
        with pytest.raises(SystemExit):
            sv.main(["-k", str(tmp_path / "kitti")] + full[:at] + full[at + 2:])
    for bad in (["--voxel-map", out], ["--poses", poses], ["--batch", "2", "--poses", poses], ["--batch", "2", "--ply", ply, "--voxel", "0.2", "--poses", poses]):
        with pytest.raises(SystemExit):
            sv.main(["-k", str(tmp_path / "kitti")] + bad)
    assert not os.path.exists(out) and not os.path.exists(ply)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _three(call, b, at, filler):
    """Frame b of a call at position `at` of a batch of 3; the other two frames hold `filler` rows that count 0 and -1."""
    xyz, color, n, counts, poses = call
    pick = lambda a, fill: None if a is None else np.stack([a[b] if j == at else np.full_like(a[b], fill) for j in range(3)])  # noqa: E731
    k = np.array([0, -1, 0], np.int32)
    k[at] = counts[b]
    return (pick(xyz, filler), pick(color, 7), pick(n, 3), k, pick(poses, 0.5))


@pytest.mark.gpu
def test_painted_and_random_cases(sv, eng):
    todo = [(p, c) for p, c, _ in cases.painted_cases().values()] + [cases.random_case(s) for s in range(50)]
    seen = set()
    for params, calls in todo:
        want = _define(sv, params, calls)
        for dtype in ("f32", "f64"):
            got, stats = _engine_rows(eng, sv, params, calls, dtype=dtype)
            assert _same(got, sv.voxel_map_rows(want, dtype=dtype))
        assert stats == (len(want["key"]), want["dropped"], False)
        world = _rig_map(params, calls)
        assert _same(_host(world.rows()), sv.voxel_map_rows(want)) and world.stats() == {"claimed": stats[0], "dropped": stats[1], "overflowed": False}
        call = calls[0]
        for b in range(call[0].shape[0]):  # each frame alone and at each position of a batch of 3
            alone = tuple(None if a is None else a[b:b + 1] for a in call)
            ref = sv.voxel_map_rows(_define(sv, params, [alone]))
            assert _same(_engine_rows(eng, sv, params, [alone])[0], ref)
            for at in range(3):
                got, stats = _engine_rows(eng, sv, params, [_three(call, b, at, params["lo"][0] + 0.5 * params["size"])])
                assert _same(got, ref, [f for f in FIELDS if not f.endswith("_seq")]) and (got["last_seq"] == at).all() and (got["first_seq"] == at).all()
            seen.add("zero" if call[3][b] == 0 else "minus" if call[3][b] < 0 else "above" if call[3][b] > call[0].shape[1] else "some")
    assert seen == {"zero", "minus", "above", "some"}  # a count above cap is cut at cap


@pytest.mark.gpu
def test_run_layouts_lane_by_lane(sv, eng):
    import torch
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    try:
        for name, (params, calls, _) in cases.painted_cases().items():
            want = sv.voxel_map_rows(_define(sv, params, calls))
            rows = {}
            for combine in (True, False):
                counters.zero_()
                eng.debug_voxel_map(combine, counters)
                rows[combine], _ = _engine_rows(eng, sv, params, calls)
                updates, atomics = counters.cpu().tolist()
                assert updates == cases.table_updates(params, calls, combine), (name, combine)
                per_update = 7 if calls[0][1] is None else 11  # n, S, m, first, last (+ C); a CAS per probe and a wavefront's claims besides
                assert atomics > updates * (per_update + 1), (name, combine)
            assert _same(rows[True], want) and _same(rows[False], want), name  # the merge changes no bit
    finally:
        eng.debug_voxel_map(True, None)


@pytest.mark.gpu
def test_probing(sv, eng):
    for slot in (500, 1023):  # colliding keys; from the last slot the probes wrap to slot 0
        cells = cases.colliding_cells(sv.voxel_map_slot_of, slot, 8)
        pts = cases.cell_points(np.repeat(cells, 3, 0))
        pts = pts[np.random.default_rng(slot).permutation(len(pts))]
        calls = [cases.one_frame(pts, np.full((len(pts), 4), 100), dtype=np.float32)]
        got, stats = _engine_rows(eng, sv, PROBE_BOX, calls)
        assert _same(got, sv.voxel_map_rows(_define(sv, PROBE_BOX, calls))) and got["count"] == 8 and (got["m"] == 3).all() and stats == (8, 0, False)
        raw = eng.voxel_map_rows(_engine_map(eng, sv, PROBE_BOX, calls)[0], sv.voxel_map_params(**PROBE_BOX), sort=False)
        assert int(raw["count"].item()) == 8 and sorted(raw["key"][:8].cpu().tolist()) == got["key"].tolist()
        if slot == 1023:  # slot order: the wrapped entries come first
            first = raw["key"][:8].cpu().numpy()
            assert (sv.voxel_map_slot_of(first, 1024) == 1023).all()


@pytest.mark.gpu
def test_capacity(sv, eng):
    rigmod = util.pkg("rig")
    full = cases.one_frame(cases.cell_points(cases.distinct_cells(512)), dtype=np.float32)
    got, stats = _engine_rows(eng, sv, BOX16, [full])
    assert got["count"] == 512 and stats == (512, 0, False) and _same(got, sv.voxel_map_rows(_define(sv, BOX16, [full])))
    world = rigmod.VoxelMap(BOX16["lo"], BOX16["hi"], BOX16["size"], 512)
    world.update(*_dev(full[:4]), full[4])
    assert world.rows()["count"] == 512 and not world.stats()["overflowed"]
    world.update(*_dev(cases.one_frame(cases.cell_points([(15, 15, 15)]))[:4]), IDENTITY[None])  # the 513th voxel
    over = world.rows()
    assert over["count"] == -1 and all(len(over[f]) == 0 for f in FIELDS) and world.stats()["overflowed"]
    assert _same(_host(over), sv.voxel_map_rows(_define(sv, BOX16, [full, cases.one_frame(cases.cell_points([(15, 15, 15)]))])))
    world.update(*_dev(full[:4]), full[4])  # sticky, and nothing faults
    assert world.rows()["count"] == -1
    with pytest.raises(RuntimeError):
        world.write_ply(os.devnull)
    world.reset()
    world.update(*_dev(full[:4]), full[4])
    assert _same(_host(world.rows()), sv.voxel_map_rows(_define(sv, BOX16, [full]))) and world.stats() == {"claimed": 512, "dropped": 0, "overflowed": False}
    # 513 voxels in one call, and an output capacity below the qualifying rows: the count is not capped
    buf, words = _engine_map(eng, sv, BOX16, [cases.one_frame(cases.cell_points(cases.distinct_cells(513)))])
    assert eng.voxel_map_rows(buf, words)["count"] == -1 and eng.voxel_map_stats(buf)[2]
    buf, words = _engine_map(eng, sv, BOX16, [full])
    raw = eng.voxel_map_rows(buf, words, capacity=100, sort=False)
    assert int(raw["count"].item()) == 512 and tuple(raw["xyz"].shape) == (100, 3) and len(set(raw["key"].cpu().tolist())) == 100
    assert int(eng.voxel_map_rows(buf, words, capacity=0, sort=False)["count"].item()) == 512
    with pytest.raises(eng.StereoError):
        eng.voxel_map_rows(buf, words, capacity=100)


@pytest.mark.gpu
def test_persistence_and_poses(sv, eng):
    rng = np.random.default_rng(21)
    params = dict(lo=(-8.0, -8.0, -2.0), hi=(8.0, 8.0, 2.0), size=1.0, capacity=512)
    B, cap = 4, 150
    xyz = rng.uniform(-6, 6, (B, cap, 3)) * (1, 1, 0.3)
    color, n = rng.integers(0, 256, (B, cap, 4)).astype(np.uint8), rng.integers(1, 9, (B, cap)).astype(np.int32)
    counts = np.array([cap, 100, cap, 7], np.int32)
    yaw = rng.uniform(-1, 1, B)
    general = np.linalg.qr(rng.normal(size=(3, 3)))[0]  # a non-planar rotation, orthogonal only up to rounding: taken as it is
    poses = {"identity": np.tile(IDENTITY, (B, 1)), "quarter": np.tile(QUARTER, (B, 1)),
             "general": np.concatenate([np.tile(general.reshape(1, 9), (B, 1)), rng.uniform(-1, 1, (B, 3))], 1),
             "odometry": sv.voxel_map_pose(rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), yaw, 0.25)}
    for name, p in poses.items():
        call = (xyz if name != "general" else xyz.astype(np.float32), color, n, counts, p)
        want = sv.voxel_map_rows(_define(sv, params, [call]))
        assert want["count"] > 50 and _same(_engine_rows(eng, sv, params, [call])[0], want), name
        two = [tuple(a[:3] for a in call), tuple(a[3:] for a in call)]  # two updates equal one, and the numbering goes on
        world = _rig_map(params, two)
        got = _host(world.rows())
        assert world.seq == 4 and _same(got, want) and got["last_seq"].max() == 3 and got["first_seq"].min() == 0, name
        assert _same(_host(world.rows(since=3, min_rows=2)), sv.voxel_map_rows(_define(sv, params, [call]), since=3, min_rows=2))
    # the occupancy map's [B,4] poses against their [B,12] expansion, as numpy and as tensors
    occ = sv.occupancy_pose(rng.uniform(-1, 1, B), rng.uniform(-1, 1, B), yaw)
    want = sv.voxel_map_rows(_define(sv, params, [(xyz, color, n, counts, sv.voxel_map_pose_words(occ))]))
    for p in (occ, _cuda(occ), _cuda(sv.voxel_map_pose_words(occ))):
        assert _same(_host(_rig_map(params, [(xyz, color, n, counts, p)]).rows()), want)


@pytest.mark.gpu
def test_reproducibility(sv, eng):
    import torch
    rng = np.random.default_rng(33)
    B, cap = 3, 2000
    xyz = rng.uniform(0.01, 15.99, (B, cap, 3)).astype(np.float32)  # ~ 490 of 512 voxels... of a box of 8 x 8 x 8 cells
    params = dict(lo=(0.0, 0.0, 0.0), hi=(16.0, 16.0, 16.0), size=2.0, capacity=512)
    call = (xyz, rng.integers(0, 256, (B, cap, 4)).astype(np.uint8), rng.integers(1, 99, (B, cap)).astype(np.int32), np.full(B, cap, np.int32), np.tile(IDENTITY, (B, 1)))
    words = sv.voxel_map_params(**params)
    want = sv.voxel_map_rows(_define(sv, params, [call, call]))
    assert want["count"] == 512
    raws = []
    for _ in range(5):
        buf = torch.full((eng.voxel_map_lib().sv_voxel_map_bytes(512) // 8,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")  # bytes 0xA5
        eng.voxel_map_clear(buf, words)
        for seq0 in (0, B):
            eng.voxel_map_insert(buf, words, *_dev(call[:4]), call[4], seq0=seq0)
        assert _same(_host(eng.voxel_map_rows(buf, words)), want)
        raw = _host(eng.voxel_map_rows(buf, words, sort=False))
        assert int(raw["count"][0]) == 512
        order = np.argsort(raw["key"][:512])
        raws.append({f: raw[f][:512][order] for f in FIELDS})
        assert _same(dict(raws[-1], count=512), want)  # the same set of rows, whatever the slot order was


def _refuse(eng, *args, rows=False):
    L = eng.voxel_map_lib()
    rc = (L.sv_voxel_map_rows_device if rows else L.sv_voxel_map_insert_device)(*args)
    return rc == SV_ERR_ARG and b"sv_voxel_map" in L.sv_last_error(None)


@pytest.mark.gpu
def test_the_c_entry_refuses(sv, eng):
    import ctypes
    import torch
    words = sv.voxel_map_params(**BOX16)
    call = cases.one_frame(cases.cell_points(cases.distinct_cells(40)), np.full((40, 4), 5), np.full(40, 2), dtype=np.float32)
    buf, _ = _engine_map(eng, sv, BOX16, [call])
    before = buf.clone()
    xyz, color, n, counts = _dev(call[:4])
    poses = _cuda(call[4])
    spec, nbytes, st = eng.voxel_map_spec(words), buf.numel() * 8, torch.cuda.current_stream().cuda_stream

    def spec_with(**kw):
        s = eng.voxel_map_spec(words)
        for k, v in kw.items():
            if k in ("lo", "hi", "reserved"):
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return ctypes.byref(s)

    good = [buf.data_ptr(), nbytes, ctypes.byref(spec), xyz.data_ptr(), 0, color.data_ptr(), n.data_ptr(), counts.data_ptr(), poses.data_ptr(), 1, 40, 1, st]
    bad = {2: [None, spec_with(size=0.0), spec_with(size=float("nan")), spec_with(capacity=0), spec_with(capacity=2 ** 26 + 1), spec_with(reserved=(3, 1)),
               spec_with(hi=(1, 0.0)), spec_with(lo=(2, float("-inf"))), spec_with(size=1e-6)],
           0: [None, buf.data_ptr() + 8], 1: [nbytes - 8, 0], 3: [None, xyz.data_ptr() + 2], 4: [2, -1], 5: [color.data_ptr() + 1], 6: [n.data_ptr() + 2],
           7: [None, counts.data_ptr() + 1], 8: [None, poses.data_ptr() + 4], 9: [-1, 65536], 10: [-1], 11: [-1, 2 ** 31 - 1]}
    for at, values in bad.items():
        for v in values:
            assert _refuse(eng, *(good[:at] + [v] + good[at + 1:])), (at, v)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)  # the map is untouched
    shapes = (("xyz", (64, 3), torch.float32), ("color", (64, 4), torch.uint8), ("cell", (64, 3), torch.int32), ("n", (64,), torch.int64), ("m", (64,), torch.int64),
              ("first_seq", (64,), torch.int32), ("last_seq", (64,), torch.int32), ("key", (64,), torch.int64), ("count", (1,), torch.int32))
    out = {k: torch.full(shape, 77, dtype=dt, device="cuda") for k, shape, dt in shapes}
    good = [buf.data_ptr(), nbytes, ctypes.byref(spec), 1, 1, 0, 0, 64] + [out[k].data_ptr() for k, _, _ in shapes] + [st]
    bad = {2: [None, spec_with(capacity=0)], 0: [None, buf.data_ptr() + 4], 1: [nbytes - 1], 6: [2], 7: [-1], 8: [None, out["xyz"].data_ptr() + 1], 9: [out["color"].data_ptr() + 2],
           10: [out["cell"].data_ptr() + 2], 11: [out["n"].data_ptr() + 4], 12: [out["m"].data_ptr() + 4], 13: [out["first_seq"].data_ptr() + 1],
           14: [out["last_seq"].data_ptr() + 3], 15: [None, out["key"].data_ptr() + 4], 16: [None, out["count"].data_ptr() + 2]}
    for at, values in bad.items():
        for v in values:
            assert _refuse(eng, *(good[:at] + [v] + good[at + 1:]), rows=True), (at, v)
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and all((t == 77).all().item() for t in out.values())  # the outputs are untouched
    L = eng.voxel_map_lib()
    assert L.sv_voxel_map_clear_device(None, nbytes, ctypes.byref(spec), st) == SV_ERR_ARG and L.sv_voxel_map_clear_device(buf.data_ptr(), nbytes, None, st) == SV_ERR_ARG
    assert L.sv_voxel_map_rows_device(*good) == 0 and out["count"].item() == 40  # and the good call goes through
    assert L.sv_voxel_map_insert_device(*(good[:3] + [None, 0, None, None, None, None, 0, 40, 0, st])) == 0  # an empty batch needs no pointer
    for kw in (dict(xyz=xyz.cpu()), dict(xyz=xyz.to(torch.float16)), dict(counts=counts.to(torch.int64)), dict(n=n[:, :3]), dict(color=color[..., :3]),
               dict(poses=np.zeros((2, 12))), dict(poses=np.zeros((1, 5))), dict(seq0=-1)):
        args = dict(dict(xyz=xyz, color=color, n=n, counts=counts, poses=call[4], seq0=0), **kw)
        with pytest.raises(ValueError):
            eng.voxel_map_insert(buf, words, **args)
    for kw in (dict(dtype="f16"), dict(min_n=0.5), dict(since=2 ** 31), dict(capacity=-1)):
        with pytest.raises(ValueError):
            eng.voxel_map_rows(buf, words, **kw)
    with pytest.raises(ValueError):
        eng.voxel_map_rows(buf[:100], words)


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    head, payload = data.split(b"end_header\n", 1)
    return head.decode("ascii").split("\n"), payload


@pytest.mark.gpu
def test_the_committed_drive_end_to_end(sv, eng, tmp_path):
    from PIL import Image
    from test_occupancy_map import H, W, _drive_frames
    n = 4
    ls, rs = _drive_frames(n)
    xyyaw = np.stack([0.8 * np.arange(n), 0.05 * np.arange(n), 0.03 * np.arange(n)], -1)
    poses = sv.voxel_map_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2])
    lo, hi = sv.cli_voxel_map_box(xyyaw)
    rigmod = util.pkg("rig")
    rig = rigmod.StereoRig(W, H)
    try:
        xyz, color, cnt, counts = rig.voxel_clouds(_cuda(ls[..., ::-1].copy()), _cuda(rs[..., ::-1].copy()), 0.2, sv.CLI_CLOUD_CROP[0], sv.CLI_CLOUD_CROP[1],
                                                   transform=(sv.CAMERA_TO_VEHICLE, None), capacity=65536)
        world = rig.voxel_map(lo, hi, 0.2, sv.CLI_VOXEL_MAP_CAPACITY)
    finally:
        rig.close()
    assert isinstance(world, rigmod.VoxelMap) and (counts > 1000).all().item()
    world.update(xyz[:3], color[:3], cnt[:3], counts[:3], poses[:3])
    world.update(xyz[3:], color[3:], cnt[3:], counts[3:], _cuda(poses[3:]))
    state = sv.voxel_map_state(world.params)
    sv.voxel_map_insert(state, xyz.cpu().numpy(), color.cpu().numpy(), cnt.cpu().numpy(), counts.cpu().numpy(), poses)
    want, got = sv.voxel_map_rows(state), _host(world.rows())
    assert want["count"] > int(counts.max().item()) and want["last_seq"].max() == 3 and (want["m"] > 1).any()  # the frames overlap, and the map grew
    assert _same(got, want) and world.stats() == {"claimed": want["count"], "dropped": state["dropped"], "overflowed": False}
    assert _same(_host(world.rows(min_rows=2, since=2)), sv.voxel_map_rows(state, min_rows=2, since=2))
    # the CLI: the same frames as PNGs, the same poses as a file
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("".join("%r %r %r\n" % tuple(float(v) for v in row) for row in xyyaw))
    out = str(tmp_path / "drive.ply")
    sv.main(["-k", str(tmp_path / "kitti"), "--batch", "3", "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt"), "--voxel-map", out])
    head, payload = _read_ply(out)
    rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert head[2] == "element vertex %d" % want["count"] and len(os.listdir(tmp_path / "ply")) == n
    assert np.array_equal(rec["xyz"].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(rec["rgb"], want["color"][:, 2::-1])
