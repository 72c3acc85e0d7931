"""A voxel map carved by the sight lines of frames (group (T)): stereo_vision.sv.voxel_map_carve against hand numbers and the per-ray model
of voxel_carve_cases, and engine.voxel_map_carve / rig.VoxelMap.carve / the CLI against the definition.  Every comparison is shape, dtype
and bits."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
import voxel_carve_cases as carve
import voxel_map_cases as cases
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_carve_cases import STATS
from voxel_map_cases import BOX16, FIELDS, IDENTITY, PROBE_BOX

SV_ERR_ARG = -1
FRESH_FIRST = np.iinfo(np.int64).max  # what voxel_map_insert's acc starts a voxel's first_seq from; its last_seq starts from -1


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


def _copy(state):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}


def _summary(sv, state):
    """What a map is compared by: its rows in f64, and (claimed, dropped, overflowed)."""
    return sv.voxel_map_rows(state, dtype="f64"), (len(state["key"]), state["dropped"], state["overflowed"])


def _next_insert(case):
    """The case's own frames - their first 40 rows at most, so that the map's capacity holds - as one more insert, and its sequence number:
    behind everything the case has numbered."""
    xyz, n, counts, poses = case["frames"]
    return (xyz, None, n, np.minimum(counts, 40), poses), sum(c[0].shape[0] for c in case["calls"]) + case["kw"].get("seq0", 0) + xyz.shape[0]


def _numpy_carve(sv, case):
    """Per case: the map before, the carve's dict, the summary behind it, and the summary behind one more insert."""
    state = _define(sv, case["params"], case["calls"])
    before = _copy(state)
    dry = sv.voxel_map_carve(state, *case["frames"], apply=False, **case["kw"])
    assert all(np.array_equal(state[k], before[k]) if isinstance(before[k], np.ndarray) else state[k] == before[k] for k in before)  # apply = 0 only reads
    res = sv.voxel_map_carve(state, *case["frames"], **case["kw"])
    assert all(np.array_equal(res[k], dry[k]) for k in res)
    carved = _summary(sv, state)
    after = _copy(state)
    call, seq = _next_insert(case)
    sv.voxel_map_insert(state, *call, seq0=seq)
    assert not state["overflowed"]  # an insert that overflows leaves `claimed` undefined on the device
    return dict(before=before, res=res, state=after, carved=carved, inserted=_summary(sv, state))


@pytest.fixture(scope="module")
def all_cases(sv):
    return carve.all_cases(sv.voxel_map_slot_of)


@pytest.fixture(scope="module")
def defined(sv, all_cases):
    """The numpy form's results per case, computed once and shared by the CPU and the GPU tests."""
    return {name: _numpy_carve(sv, case) for name, case in all_cases.items()}


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_hand_case(sv):
    """Sensor cell (2, 2, 2), one row of weight 3 in cell (8, 2, 2), margin 1: the steps visit x = 3, 4, 5, 6 at y = z = 2."""
    state = _define(sv, BOX16, [cases.one_frame(cases.cell_points([(4, 2, 2), (6, 2, 2), (6, 3, 2)]), None, [1, 4, 2])])
    key_a, key_b, key_c = 4 | 2 << 20 | 2 << 40, 6 | 2 << 20 | 2 << 40, 6 | 3 << 20 | 2 << 40
    assert state["key"].tolist() == [key_a, key_b, key_c] and state["n"].tolist() == [1, 4, 2]
    xyz, n, counts, poses = np.array([[[8.5, 2.5, 2.5]]]), np.array([[3]], np.int32), np.array([1], np.int32), IDENTITY[None]
    got = sv.voxel_map_carve(state, xyz, n, counts, poses, origin=(2.5, 2.5, 2.5), seq0=1, reach=16, margin=1, min_miss=3, ratio=256)
    assert [got[k] for k in STATS] == [1, 4, 2, 1]
    assert got["key"].tolist() == [key_a, key_b] and got["miss"].tolist() == [3, 3] and got["key"].dtype == got["miss"].dtype == np.int64
    # A (256 * 3 >= 256 * 1) is a tombstone: its row stays, emptied; B (256 * 3 < 256 * 4) and C are as they were
    assert state["key"].tolist() == [key_a, key_b, key_c] and state["n"].tolist() == [0, 4, 2] and state["m"].tolist() == [0, 1, 1]
    assert state["S"].tolist() == [[0, 0, 0], [4 * 32768] * 3, [2 * 32768] * 3] and state["C"].tolist() == [[0] * 4] * 3
    assert state["first_seq"].tolist() == [FRESH_FIRST, 0, 0] and state["last_seq"].tolist() == [-1, 0, 0]
    rows = sv.voxel_map_rows(state)
    assert rows["key"].tolist() == [key_b, key_c] and rows["count"] == 2  # skipped at min_n = 1
    # margin 0 reaches x = 7 as well, margin 4 stops at x = 3; the same frame numbered 0 counts against nothing
    assert sv.voxel_map_carve(state, xyz, n, counts, poses, origin=(2.5, 2.5, 2.5), seq0=1, reach=16, margin=0, apply=False)["steps"] == 5
    assert [sv.voxel_map_carve(state, xyz, n, counts, poses, origin=(2.5, 2.5, 2.5), seq0=1, reach=16, margin=4, apply=False)[k] for k in STATS] == [1, 1, 0, 0]
    assert [sv.voxel_map_carve(state, xyz, n, counts, poses, origin=(2.5, 2.5, 2.5), seq0=0, reach=16, apply=False)[k] for k in STATS] == [1, 4, 0, 0]
    # the emptied voxel reads as last seen at 0: a second carve counts against it, and carves it again, with nothing more to take
    again = sv.voxel_map_carve(state, xyz, n, counts, poses, origin=(2.5, 2.5, 2.5), seq0=1, reach=16, min_miss=3, ratio=256)
    assert [again[k] for k in STATS] == [1, 4, 2, 1] and state["n"].tolist() == [0, 4, 2]
    assert carve.model_carve(BOX16, {key_a: (1, 0), key_b: (4, 0), key_c: (2, 0)}, (xyz, n, counts, poses), origin=(2.5, 2.5, 2.5), seq0=1, reach=16, margin=1,
                             min_miss=3, ratio=256) == (dict(zip(STATS, (1, 4, 2, 1))), {key_a: 3, key_b: 3}, {key_a})


def test_the_numpy_form_against_the_model(sv, all_cases, defined):
    assert len(all_cases) >= 30
    for name, case in all_cases.items():
        d = defined[name]
        stats, miss, carved = carve.model_carve(case["params"], carve.voxels_of(d["before"]), case["frames"], **case["kw"])
        assert [d["res"][k] for k in STATS] == [stats[k] for k in STATS], (name, d["res"], stats)
        assert d["res"]["key"].tolist() == sorted(miss) and d["res"]["miss"].tolist() == [miss[k] for k in sorted(miss)], name
        assert d["res"]["key"].dtype == d["res"]["miss"].dtype == np.int64
        # the state behind the carve: the same rows; a carved voxel emptied to what an insert starts from, every other one untouched
        before, after = d["before"], d["state"]
        gone = np.isin(before["key"], sorted(carved))
        assert np.array_equal(after["key"], before["key"]) and int(gone.sum()) == stats["carved"], name
        for f, fresh in (("n", 0), ("S", 0), ("C", 0), ("m", 0), ("first_seq", FRESH_FIRST), ("last_seq", -1)):
            assert (after[f][gone] == fresh).all() and np.array_equal(after[f][~gone], before[f][~gone]), (name, f)
        assert (after["dropped"], after["overflowed"]) == (before["dropped"], before["overflowed"]) and d["carved"][1][0] == len(before["key"])
        assert d["carved"][0]["count"] == int((before["n"] > 0).sum()) - stats["carved"], name


def test_direction_and_rounding(sv, defined):
    case = carve.direction_case()
    exact, differ = carve.rounding_census(case)
    assert exact > 100 and differ > 100  # half-way steps on an axis that moves down, and quotients that floor and truncate apart
    res = defined["directions"]["res"]
    assert res["rays"] == 386 + 5 and res["steps"] == 386 * 3 + 5 * 5 and res["touched"] == 7 ** 3 - 1  # every inner cell but the sensor's own
    # the ray to (4, 6, 8): d = (-4, -2, 0); k = 1 and k = 3 lie half way on y and round up: (7, 8, 8), (6, 7, 8), (5, 7, 8)
    assert carve.ray_cells((8, 8, 8), (4, 6, 8), 0)[0] == [(7, 8, 8), (6, 7, 8), (5, 7, 8)]
    assert carve.ray_cells((8, 8, 8), (5, 4, 7), 0)[0] == [(7, 7, 8), (7, 6, 8), (6, 5, 7)]  # d = (-3, -4, -1): -3/4 -> -1, -1/4 -> 0


def test_ray_limits(sv, defined):
    # rows at nst = 5 (= reach), 6, 0, 5, 6 from the sensor: three rays whatever the margin; the two of five steps walk 4 - margin cells
    for margin, steps, touched in ((0, 8, 4), (1, 6, 3), (3, 2, 1), (4, 0, 0), (7, 0, 0), (255, 0, 0)):
        res = defined["limits_margin_%d" % margin]["res"]
        assert [res[k] for k in STATS] == [3, steps, touched, touched], margin
    state = _define(sv, BOX16, [cases.one_frame(cases.cell_points(carve.X_LINE))])
    row = lambda x: carve.frames_of(cases.cell_points([(x, 8, 8)]))  # noqa: E731
    kw = dict(origin=(2.5, 8.5, 8.5), seq0=1, margin=0, apply=False)
    assert [sv.voxel_map_carve(state, *row(7), reach=r, **kw)["rays"] for r in (4, 5, 6)] == [0, 1, 1]
    assert [sv.voxel_map_carve(state, *row(2), reach=1, **kw)[k] for k in STATS] == [1, 0, 0, 0]  # nst = 0: a ray without steps
    assert [sv.voxel_map_carve(state, *row(3), reach=1, **kw)[k] for k in STATS] == [1, 0, 0, 0]  # nst = 1: its only cells are the two ends


def test_the_sequence_guard(sv, defined):
    d = defined["sequence_guard"]
    assert d["before"]["last_seq"].tolist() == [0, 1, 2] and d["res"]["key"].tolist() == [5 | 8 << 20 | 8 << 40] and d["res"]["miss"].tolist() == [1]
    d = defined["sequence_batch"]  # carved with the batch that built it
    at = d["before"]["key"].tolist().index(5 | 8 << 20 | 8 << 40)
    assert d["before"]["last_seq"][at] == 0 and d["res"]["key"].tolist() == [5 | 8 << 20 | 8 << 40] and d["res"]["miss"].tolist() == [2]  # frame 1's two rays
    assert d["res"]["rays"] == 4 and d["carved"][0]["count"] == len(d["before"]["key"]) - 1


def test_wide_sums(sv, defined):
    big = 2 ** 31 - 1
    assert defined["miss_above_2_32"]["res"]["miss"].tolist() == [5 * big] and 5 * big > 2 ** 32 and defined["miss_above_2_32"]["res"]["carved"] == 1
    assert defined["ratio_exact"]["res"]["miss"].tolist() == [6, 6] and defined["ratio_exact"]["res"]["carved"] == 2
    assert defined["ratio_one_below"]["res"]["miss"].tolist() == [5, 5] and defined["ratio_one_below"]["res"]["carved"] == 0
    assert defined["min_miss_at"]["res"]["carved"] == 2 and defined["min_miss_above"]["res"]["carved"] == 0 and defined["min_miss_above"]["res"]["touched"] == 2


def test_who_casts(sv, all_cases, defined):
    for name in all_cases:
        if name.startswith(("sensor_on", "sensor_outside", "pose_not_finite")):
            assert [defined[name]["res"][k] for k in STATS] == [0, 0, 0, 0], name
    inside, turned = defined["sensor_inside_float64"]["res"], defined["quarter_turn_float64"]["res"]
    assert inside["rays"] > 40 and inside["carved"] > 0 and all(np.array_equal(inside[k], turned[k]) for k in inside)
    assert defined["counts_zero_and_negative"]["res"]["rays"] == 0
    assert defined["straddling_rows"]["res"]["rays"] > 513 and 0 < defined["straddling_rows"]["res"]["carved"] < defined["straddling_rows"]["res"]["touched"]


def test_a_tombstone_lives_on(sv, defined):
    """Carve B of the chain A, B, C: look up, insert into and match against what is left, then prune."""
    case, (a, b, c) = carve.chain_case(sv.voxel_map_slot_of)
    slots = sv.voxel_map_slots(PROBE_BOX["capacity"])
    assert len({int(sv.voxel_map_slot_of(carve.key_of(v), slots)) for v in (a, b, c)}) == 1
    state = _copy(defined["probe_chain"]["state"])
    assert defined["probe_chain"]["res"]["key"].tolist() == [carve.key_of(b)] and len(state["key"]) == 3
    rows = sv.voxel_map_rows(state)
    assert sorted(rows["key"].tolist()) == sorted([carve.key_of(a), carve.key_of(c)])
    frame = carve.frames_of(cases.cell_points([b, c]), [7, 9])
    hit = sv.voxel_map_match(state, *frame[:3], IDENTITY[None, None])
    assert hit["inside"].tolist() == [[2]] and hit["hits"].tolist() == [[1]] and hit["weight"].tolist() == [[9]]  # C is found, B is not there
    sv.voxel_map_insert(state, frame[0], None, frame[1], frame[2], frame[3], seq0=9)
    fresh = _define(sv, PROBE_BOX, [cases.one_frame(cases.cell_points([b]), None, [7])])
    at = state["key"].tolist().index(carve.key_of(b))
    assert len(state["key"]) == 3 and all(np.array_equal(state[f][at], fresh[f][0]) for f in ("n", "S", "C", "m")) and state["n"][at] == 7
    assert (state["first_seq"][at], state["last_seq"][at]) == (9, 9)  # reborn: what a fresh voxel inserted at 9 holds
    # carve then prune: the emptied voxels are dropped as filtered, and the rows stay
    d = defined["straddling_rows"]
    pruned = sv.voxel_map_state(d["state"]["params"])
    stats = sv.voxel_map_carry(pruned, d["state"])
    assert stats["filtered"] == d["res"]["carved"] > 0 and len(pruned["key"]) == len(d["state"]["key"]) - d["res"]["carved"] == stats["carried"]
    assert _same(sv.voxel_map_rows(pruned, dtype="f64"), d["carved"][0])


def test_an_overflowed_map(sv):
    case = carve.overflowed_case()
    state = _define(sv, case["params"], case["calls"])
    before = _copy(state)
    res = sv.voxel_map_carve(state, *case["frames"], **case["kw"])
    assert [res[k] for k in STATS] == [-1, 0, 0, 0] and len(res["key"]) == len(res["miss"]) == 0 and state["overflowed"]
    assert all(np.array_equal(state[k], before[k]) for k in before if isinstance(before[k], np.ndarray))


def test_refusals(sv, tmp_path):
    state = _define(sv, BOX16, [cases.one_frame(cases.cell_points([(3, 4, 5)]))])
    before = _copy(state)
    good = dict(xyz=np.zeros((1, 4, 3)), n=None, counts=np.array([4], np.int32), poses=IDENTITY[None])
    for kw in (dict(xyz=np.zeros((1, 4, 2))), dict(xyz=np.zeros((1, 4, 3), np.int32)), dict(counts=np.zeros(2, np.int32)), dict(n=np.zeros((1, 3), np.int32)),
               dict(poses=np.zeros((1, 4))), dict(origin=(0.0, 0.0)), dict(origin=(0.0, np.nan, 0.0)), dict(origin=(0.0, np.inf, 0.0)), dict(origin=None),
               dict(seq0=-1), dict(seq0=2 ** 31 - 1), dict(seq0=0.5), dict(reach=0), dict(reach=1024), dict(reach=2.5), dict(margin=-1), dict(margin=256),
               dict(min_miss=0), dict(min_miss=2 ** 63), dict(ratio=-1), dict(ratio=65536), dict(apply=2), dict(reach=True)):
        with pytest.raises(ValueError):
            sv.voxel_map_carve(state, **dict(good, **kw))
    assert all(np.array_equal(state[k], before[k]) for k in before if isinstance(before[k], np.ndarray))
    assert sv.voxel_map_carve(state, **good, seq0=2 ** 31 - 2, reach=1023, margin=255, min_miss=2 ** 63 - 1, ratio=65535)["rays"] == 0
    # rig.VoxelMap on "cpu" runs the definition: [B,4] poses, seq0 = the frames just added, reach in metres
    cpu = util.pkg("rig").VoxelMap(device="cpu", **dict(BOX16, size=0.5))
    far = cases.one_frame(np.array([[6.2, 3.2, 1.2]]))
    cpu.update(*far[:4], np.array([[0.0, 0.0, 1.0, 0.0]]))
    near = cases.one_frame(np.array([[7.2, 3.2, 1.2], [7.2, 3.2, 1.2]]))
    cpu.update(*near[:4], np.array([[0.0, 0.0, 1.0, 0.0]]))
    res = cpu.carve(near[0], near[2], near[3], np.array([[0.0, 0.0, 1.0, 0.0]]), origin=(0.2, 3.2, 1.2), reach_m=8.0)
    assert [res[k] for k in STATS] == [2, 2 * (14 - 1 - 1), 1, 1] and cpu.stats()["claimed"] == 2 and cpu.rows()["count"] == 1
    key, miss = cpu.touched(res)
    assert key.tolist() == [12 | 6 << 20 | 2 << 40] and miss.tolist() == [2]
    assert [cpu.carve(near[0], near[2], near[3], np.array([[0.0, 0.0, 1.0, 0.0]]), origin=(0.2, 3.2, 1.2), reach_m=6.5)[k] for k in STATS] == [0, 0, 0, 0]  # 14 cells > 13
    cpu.carve(near[0], near[2], near[3], np.array([[0.0, 0.0, 1.0, 0.0]]), prune=True)
    assert cpu.stats()["claimed"] == 1
    for kw in (dict(reach_m=0.0), dict(reach_m=512.0), dict(reach_m=np.nan), dict(margin=256), dict(min_miss=0), dict(ratio=-1)):
        with pytest.raises(ValueError):
            cpu.carve(near[0], near[2], near[3], np.array([[0.0, 0.0, 1.0, 0.0]]), **kw)
    # the CLI's argument errors
    poses_file, ply, out = str(tmp_path / "poses.txt"), str(tmp_path / "ply"), str(tmp_path / "drive.ply")
    with open(poses_file, "w") as f:
        f.write("0 0 0\n")
    full = ["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", ply, "--voxel", "0.2", "--poses", poses_file]
    for bad in (full + ["--voxel-carve", "10"], full + ["--voxel-map", out, "--voxel-carve", "x"], full + ["--voxel-map", out, "--voxel-carve", "10,2,0,1"],
                full + ["--voxel-map", out, "--voxel-carve", "0"], full + ["--voxel-map", out, "--voxel-carve", "205"], full + ["--voxel-map", out, "--voxel-carve", "10,0"],
                full + ["--voxel-map", out, "--voxel-carve", "10,2,65536"], full + ["--voxel-map", out, "--voxel-carve", "10,1.5"]):
        with pytest.raises(SystemExit):
            sv.main(bad)
    assert not os.path.exists(out) and not os.path.exists(ply)
    assert sv.cli_voxel_carve_spec(204.6, 1, 65535, 0.2) == (204.6, 1, 65535) and sv.cli_voxel_carve_text(dict(zip(STATS, (4, 3, 2, 1)))) == "rays 4, steps 3, touched 2, carved 1"


def _aligned(words, fill, offset_words=0):
    """A host int64 array of `words` words that starts 16-byte aligned plus offset_words words."""
    raw = np.full(words + 3, fill, np.int64)
    skip = ((-raw.ctypes.data) % 16) // 8 + offset_words
    return raw, raw[skip:skip + words]


def test_the_c_entry_refuses(sv, eng):
    """Every check of the C entry runs before any HIP call: host memory stands in for the device buffers, and stays as it was."""
    L = eng.voxel_carve_lib()
    spec = eng.voxel_map_spec(sv.voxel_map_params(**BOX16))
    need, slots = L.sv_voxel_map_bytes(512), L.sv_voxel_map_slots(512)
    assert slots == 1024 and need == 32 + 1024 * 88 + 16
    (_, buf), (_, miss), (_, stats) = _aligned(need // 8, 5), _aligned(slots, 7), _aligned(4, 7)
    (_, xyz), (_, n), (_, counts), (_, poses) = _aligned(3 * 4, 0), _aligned(2, 1), _aligned(1, 0), _aligned(12, 0)
    origin = np.zeros(3)
    good = dict(map=buf.ctypes.data, map_bytes=need, spec=spec, xyz=xyz.ctypes.data, dtype=1, n=n.ctypes.data, counts=counts.ctypes.data, poses=poses.ctypes.data,
                origin=origin.ctypes.data, batch=1, cap=4, seq0=0, reach=16, margin=1, min_miss=1, ratio=0, apply=1, miss=miss.ctypes.data, stats=stats.ctypes.data)

    def call(**change):
        a = dict(good, **change)
        return L.sv_voxel_carve_device(a["map"], a["map_bytes"], None if a["spec"] is None else ctypes.byref(a["spec"]), a["xyz"], a["dtype"], a["n"], a["counts"], a["poses"],
                                       a["origin"], a["batch"], a["cap"], a["seq0"], a["reach"], a["margin"], a["min_miss"], a["ratio"], a["apply"], a["miss"], a["stats"], None)

    def spec_with(**words):
        s = eng.voxel_map_spec(sv.voxel_map_params(**BOX16))
        for k, v in words.items():
            if k in ("lo", "hi"):
                getattr(s, k)[0] = v
            elif k == "reserved":
                s.reserved[3] = v
            else:
                setattr(s, k, v)
        return s

    bad = [dict(spec=None), dict(map=None), dict(map=good["map"] + 8), dict(map_bytes=need - 8), dict(map_bytes=0)]
    bad += [dict(spec=spec_with(**w)) for w in (dict(reserved=1), dict(size=0.0), dict(size=float("nan")), dict(size=float("inf")), dict(lo=float("-inf")),
                                                dict(hi=float("nan")), dict(lo=16.0), dict(size=1e-6), dict(capacity=0), dict(capacity=2 ** 26 + 1))]
    bad += [dict(dtype=2), dict(dtype=-1), dict(batch=-1), dict(batch=65536), dict(cap=-1), dict(seq0=-1), dict(seq0=2 ** 31 - 1), dict(seq0=2 ** 31 - 3, batch=3)]
    bad += [dict(reach=0), dict(reach=1024), dict(reach=-5), dict(margin=-1), dict(margin=256), dict(min_miss=0), dict(min_miss=-2 ** 63), dict(ratio=-1),
            dict(ratio=65536), dict(apply=2), dict(apply=-1)]
    bad += [dict(counts=None), dict(poses=None), dict(xyz=None), dict(xyz=good["xyz"] + 4), dict(n=good["n"] + 2), dict(counts=good["counts"] + 1),
            dict(poses=good["poses"] + 4), dict(miss=None), dict(miss=good["miss"] + 4), dict(stats=good["stats"] + 4), dict(origin=None)]
    bad += [dict(origin=np.array(o).ctypes.data) for o in ((np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, -np.inf))]
    bad += [dict(miss=good["map"]), dict(miss=good["map"] + need - 8), dict(miss=good["map"] - 8 * slots + 8), dict(stats=good["map"] + 64), dict(stats=good["map"] + need - 8),
            dict(stats=good["miss"] + 8), dict(stats=good["miss"] + 8 * slots - 8)]
    for change in bad:
        eng.lib().sv_last_error(None)
        assert call(**change) == SV_ERR_ARG, change
        text = eng.lib().sv_last_error(None)
        assert text and b"sv_voxel_carve" in text, change
    assert (buf == 5).all() and (miss == 7).all() and (stats == 7).all()


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\(?\b(sv_\w*carve\w*)\)?\s*\(", src) == ["sv_voxel_carve_device"]
    assert text.index("/* ---- (S)") < text.index("/* ---- (T)") < text.index("/* ---- (A)") and " *  (T) " in text
    assert set(util.pkg("engine").STAGE_SIGNATURES["voxel_carve"]) == {"sv_voxel_carve_device"}
    build = util.pkg("build")
    assert "voxel_carve_kernels.hip" in build.SOURCES and "voxel_carve.cpp" in build.SOURCES and "voxel_carve_kernels.h" in build.HEADERS
    assert "voxel_map_carve" in sv.__doc__ and "(T)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_carve_kernels.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert "asm" not in code and "float" not in re.sub(r"const float \*p|static_cast<const float \*>", "", code) and code.count("atomicAdd(a.miss") == 1
    assert len(re.findall(r"\batomic\w*\(", code)) == 3  # the miss, and one flush of the counters per workgroup in two kernels
    # slot_of, the transform, the kept rule, the cell rule and the read-only probe are the map's own, defined once; the match uses the same probe
    header = cases.check_map_table(build)
    match = open(os.path.join(build.CSRC, "voxel_match_kernels.hip")).read()
    assert cases.squeeze("if (k == VMAP_EMPTY) return") in header and code.count("vmap_find(") == 1 and match.count("vmap_find(") == 1
    assert code.count("vmap_slot_of(") == 1 and code.count("vmap_rows_of(") == 1
    assert code.count("vmap_cell(") == 2  # the sensor and the row
    # the weight's part of the kept rule stays with the insert's, restated: the same text in both files
    insert = open(os.path.join(build.CSRC, "voxel_map_kernels.hip")).read()
    for line in ("if (a.weight) wt = a.weight[o];", "keep = wt > 0;"):
        assert cases.squeeze(line) in cases.squeeze(source) and cases.squeeze(line) in cases.squeeze(insert), line


# ---------------------------------------------------------------------------------------------------------------- GPU

def _host(rows):
    return {k: v if k == "count" else v.cpu().numpy() for k, v in rows.items()}


def _engine_map(eng, sv, params, calls):
    words = sv.voxel_map_params(**params)
    buf, seq = eng.voxel_map_new(words), 0
    for call in calls:
        eng.voxel_map_insert(buf, words, *(None if a is None else _cuda(a) for a in call[:4]), call[4], seq0=seq)
        seq += call[0].shape[0]
    return buf, words


def _engine_carve(eng, buf, words, case, **more):
    xyz, n, counts, poses = case["frames"]
    return eng.voxel_map_carve(buf, words, _cuda(xyz), None if n is None else _cuda(n), _cuda(counts), poses, **dict(case["kw"], **more))


def _touched(eng, buf, words, res):
    key, miss = eng.voxel_carve_touched(buf, words, res.miss)
    return key.cpu().numpy(), miss.cpu().numpy()


def _same_arrays(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_the_device_against_the_numpy_form(sv, eng, all_cases, defined):
    import torch
    for name, case in all_cases.items():
        want = defined[name]
        buf, words = _engine_map(eng, sv, case["params"], case["calls"])
        twin = buf.clone()
        # apply = 0 leaves the map's buffer byte for byte as it was
        dry = _engine_carve(eng, buf, words, case, apply=False)
        assert torch.equal(buf, twin), name
        assert dry.stats.dtype == dry.miss.dtype == torch.int64 and tuple(dry.stats.shape) == (4,) and tuple(dry.miss.shape) == (sv.voxel_map_slots(words["capacity"]),)
        res = _engine_carve(eng, buf, words, case)
        assert res.stats.cpu().tolist() == [want["res"][k] for k in STATS], (name, res.stats.cpu().tolist(), want["res"])
        assert torch.equal(res.stats, dry.stats) and torch.equal(res.miss, dry.miss), name
        key, miss = _touched(eng, buf, words, res)
        assert _same_arrays(key, want["res"]["key"]) and _same_arrays(miss, want["res"]["miss"]), name
        assert _same(_host(eng.voxel_map_rows(buf, words, dtype="f64")), want["carved"][0]) and eng.voxel_map_stats(buf) == want["carved"][1], name
        # the same call into an equal map: equal bytes, whatever the schedule was
        again = _engine_carve(eng, twin, words, case)
        assert torch.equal(again.stats, res.stats) and torch.equal(again.miss, res.miss), name
        # and the map carries on: one more insert
        call, seq = _next_insert(case)
        eng.voxel_map_insert(buf, words, *(None if a is None else _cuda(a) for a in call[:4]), call[4], seq0=seq)
        assert _same(_host(eng.voxel_map_rows(buf, words, dtype="f64")), want["inserted"][0]) and eng.voxel_map_stats(buf) == want["inserted"][1], name


@pytest.mark.gpu
def test_the_chain_on_the_device(sv, eng, defined):
    """A, B, C lie in three slots in a row; B is carved and its key stays, so C is still found, B is reborn by an insert, and claimed stays 3."""
    case, (a, b, c) = carve.chain_case(sv.voxel_map_slot_of)
    buf, words = _engine_map(eng, sv, case["params"], case["calls"])
    start = int(sv.voxel_map_slot_of(carve.key_of(a), 1024))
    res = _engine_carve(eng, buf, words, case)
    table = buf[4:4 + 11 * 1024].view(1024, 11).cpu().numpy()
    assert table[start:start + 4, 0].tolist() == [carve.key_of(a), carve.key_of(b), carve.key_of(c), -1]
    assert table[start + 1, 1:].tolist() == [0] * 9 + [0xFFFFFFFF] and table[start + 2, 1] == 5 and res.miss.cpu().numpy()[start:start + 3].tolist() == [0, 2, 0]
    assert res.stats.cpu().tolist() == [1, 3, 1, 1] and eng.voxel_map_stats(buf) == (3, 0, False)
    frame = carve.frames_of(cases.cell_points([b, c]), [7, 9])
    hit = eng.voxel_map_match(buf, words, _cuda(frame[0]), _cuda(frame[1]), _cuda(frame[2]), IDENTITY[None, None])
    assert hit.inside.cpu().tolist() == [[2]] and hit.hits.cpu().tolist() == [[1]] and hit.weight.cpu().tolist() == [[9]]
    eng.voxel_map_insert(buf, words, _cuda(frame[0]), None, _cuda(frame[1]), _cuda(frame[2]), frame[3], seq0=9)
    state = _copy(defined["probe_chain"]["state"])
    sv.voxel_map_insert(state, frame[0], None, frame[1], frame[2], frame[3], seq0=9)
    assert _same(_host(eng.voxel_map_rows(buf, words, dtype="f64")), sv.voxel_map_rows(state, dtype="f64")) and eng.voxel_map_stats(buf) == (3, 0, False)
    table = buf[4:4 + 11 * 1024].view(1024, 11).cpu().numpy()
    assert table[start + 1].tolist() == [carve.key_of(b), 7, 7 * 32768, 7 * 32768, 7 * 32768, 0, 0, 0, 0, 1, 9 | 9 << 32]  # what a fresh voxel would hold


def _rig_pair(box, calls):
    rigmod = util.pkg("rig")
    pair = [rigmod.VoxelMap(box["lo"], box["hi"], box["size"], box["capacity"], device=d) for d in ("cuda", "cpu")]
    for call in calls:
        pair[0].update(*(None if a is None else _cuda(a) for a in call[:4]), call[4])
        pair[1].update(*call)
    return pair


@pytest.mark.gpu
def test_the_method_of_the_map_on_both_devices(sv, eng):
    """update, then carve with the same frames ([B,4] poses, seq0 left to the map), on the device and on the CPU; then prune."""
    box = dict(lo=(-8.0, -8.0, -2.0), hi=(8.0, 8.0, 2.0), size=0.5, capacity=2048)
    rng = np.random.default_rng(21)

    def call(at):
        xyz = (rng.uniform(-9, 9, (2, 300, 3)) * [1, 1, 0.25] + [at, 0.0, 0.0]).astype(np.float32)
        return xyz, None, rng.integers(1, 9, (2, 300)).astype(np.int32), np.array([300, 211], np.int32), np.array([[at, 0.1, 1.0, 0.0], [at + 0.3, -0.2, 0.6, 0.8]])

    gpu, cpu = _rig_pair(box, [call(0.0), call(0.5)])
    last = call(1.0)
    gpu.update(*(None if a is None else _cuda(a) for a in last[:4]), last[4])
    cpu.update(*last)
    kw = dict(origin=(0.25, 0.0, 0.3), reach_m=6.0, margin=1, min_miss=3, ratio=64)
    got, want = gpu.carve(_cuda(last[0]), _cuda(last[2]), _cuda(last[3]), last[4], **kw), cpu.carve(last[0], last[2], last[3], last[4], **kw)
    assert got.stats.cpu().tolist() == [want[k] for k in STATS] and want["carved"] > 10 and want["touched"] > want["carved"]
    key, miss = gpu.touched(got)
    assert _same_arrays(key.cpu().numpy(), want["key"]) and _same_arrays(miss.cpu().numpy(), want["miss"])
    assert all(_same_arrays(a.numpy(), b) for a, b in zip(cpu.touched(want), (want["key"], want["miss"])))
    assert gpu.stats() == cpu.stats() and _same(_host(gpu.rows(dtype="f64")), _host(cpu.rows(dtype="f64")))
    kept = got.miss.data_ptr()
    # an earlier batch, named by its seq0, carved and pruned in one call: the tensor per slot is the one from before
    first = call(0.0)
    got, want = (gpu.carve(_cuda(first[0]), _cuda(first[2]), _cuda(first[3]), first[4], seq0=2, prune=True, **kw),
                 cpu.carve(first[0], first[2], first[3], first[4], seq0=2, prune=True, **kw))
    assert got.stats.cpu().tolist() == [want[k] for k in STATS] and got.miss.data_ptr() == kept
    assert gpu.stats() == cpu.stats() and gpu.seq == cpu.seq == 6 and _same(_host(gpu.rows(dtype="f64")), _host(cpu.rows(dtype="f64")))
    with pytest.raises(ValueError):
        gpu.carve(_cuda(first[0]), _cuda(first[2]), _cuda(first[3]), first[4], reach_m=512.0)


@pytest.mark.gpu
def test_carve_then_prune(sv, eng, all_cases, defined):
    case, want = all_cases["straddling_rows"], defined["straddling_rows"]
    buf, words = _engine_map(eng, sv, case["params"], case["calls"])
    res = _engine_carve(eng, buf, words, case)
    claimed = eng.voxel_map_stats(buf)[0]
    into = eng.voxel_map_new(words)
    stats = eng.voxel_map_carry(into, words, buf, words).cpu().tolist()
    carved = int(res.stats[3])
    assert carved == want["res"]["carved"] > 0 and stats[1] == carved and stats[0] == stats[3] == claimed - carved == eng.voxel_map_stats(into)[0]
    assert _same(_host(eng.voxel_map_rows(into, words, dtype="f64")), want["carved"][0])


@pytest.mark.gpu
def test_an_overflowed_map_on_the_device(sv, eng):
    import torch
    case = carve.overflowed_case()
    buf, words = _engine_map(eng, sv, case["params"], case["calls"])
    before = buf.clone()
    res = _engine_carve(eng, buf, words, case)
    assert res.stats.cpu().tolist() == [-1, 0, 0, 0] and not res.miss.any().item() and torch.equal(buf, before) and eng.voxel_map_stats(buf)[2]


@pytest.mark.gpu
def test_the_c_entry_accepts(sv, eng, all_cases, defined):
    """The call the refusals start from, taken: with stats and without, and with a miss buffer that starts on an odd word."""
    import torch
    L = eng.voxel_carve_lib()
    case, want = all_cases["straddling_rows"], defined["straddling_rows"]
    xyz, n, counts, poses = (_cuda(a) for a in case["frames"])
    origin = np.array(case["kw"]["origin"], np.float64)
    for odd, with_stats in ((0, True), (1, True), (1, False)):
        buf, words = _engine_map(eng, sv, case["params"], case["calls"])
        spec = eng.voxel_map_spec(words)
        room = torch.full((1024 + 4,), 7, dtype=torch.int64, device="cuda")
        stats = torch.full((6,), 7, dtype=torch.int64, device="cuda")
        assert room.data_ptr() % 16 == 0
        rc = L.sv_voxel_carve_device(buf.data_ptr(), buf.numel() * 8, ctypes.byref(spec), xyz.data_ptr(), 1, n.data_ptr(), counts.data_ptr(), poses.data_ptr(),
                                     origin.ctypes.data, 3, xyz.shape[1], 1, 16, 1, 6, 300, 1, room.data_ptr() + 8 * (1 + odd), stats.data_ptr() if with_stats else None,
                                     torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        room = room.cpu().numpy()
        assert room[:1 + odd].tolist() == [7] * (1 + odd) and room[1 + odd + 1024:].tolist() == [7] * (3 - odd)  # nothing outside its words
        miss = torch.from_numpy(room[1 + odd:1 + odd + 1024].copy()).cuda()
        key, got = eng.voxel_carve_touched(buf, words, miss)
        assert _same_arrays(key.cpu().numpy(), want["res"]["key"]) and _same_arrays(got.cpu().numpy(), want["res"]["miss"])
        assert stats.cpu().tolist() == ([want["res"][k] for k in STATS] if with_stats else [7] * 4) + [7, 7]
        assert _same(_host(eng.voxel_map_rows(buf, words, dtype="f64")), want["carved"][0])
    for kw in (dict(reach=0), dict(reach=1024), dict(margin=256), dict(min_miss=0), dict(ratio=65536), dict(apply=2), dict(seq0=-1), dict(origin=(0.0, np.nan, 0.0)),
               dict(origin=(0.0, 0.0)), dict(miss=torch.zeros(1023, dtype=torch.int64, device="cuda")), dict(miss=torch.zeros(1024, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            eng.voxel_map_carve(buf, words, xyz, n, counts, case["frames"][3], **kw)
    with pytest.raises(ValueError):
        eng.voxel_map_carve(buf, words, xyz, n[:, :5], counts, case["frames"][3])
    with pytest.raises(ValueError):
        eng.voxel_carve_touched(buf, words, miss[:1000])


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    at = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:at].decode().splitlines(), data[at:]


@pytest.mark.gpu
def test_cli_voxel_carve(sv, eng, tmp_path, capsys):
    """--voxel-carve over two batches against the same sequence driven through the CPU object."""
    from PIL import Image
    from test_occupancy_map import H, W, _drive_frames
    n = 4
    ls, rs = _drive_frames(n)
    xyyaw = np.array([[0.0, 0.0, 0.0], [0.8, 0.05, 0.03], [1.6, 0.1, 0.06], [2.4, 0.1, 0.09]])
    poses = sv.voxel_map_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2])
    lo, hi = sv.cli_voxel_map_box(xyyaw)
    rigmod = util.pkg("rig")
    rig = rigmod.StereoRig(W, H)
    try:
        cloud = rig.voxel_clouds(_cuda(ls[..., ::-1].copy()), _cuda(rs[..., ::-1].copy()), 0.2, sv.CLI_CLOUD_CROP[0], sv.CLI_CLOUD_CROP[1],
                                 transform=(sv.CAMERA_TO_VEHICLE, None), capacity=65536)
    finally:
        rig.close()
    xyz, color, cnt, counts = (t.cpu().numpy() for t in cloud)
    world = rigmod.VoxelMap(lo, hi, 0.2, sv.CLI_VOXEL_MAP_CAPACITY, device="cpu")
    events = []
    for i in (0, 2):
        world.update(xyz[i:i + 2], color[i:i + 2], cnt[i:i + 2], counts[i:i + 2], poses[i:i + 2])
        res = world.carve(xyz[i:i + 2], cnt[i:i + 2], counts[i:i + 2], poses[i:i + 2], reach_m=15.0, min_miss=2, ratio=64)
        events.append("voxel map carved after frame %d: %s" % (i + 1, sv.cli_voxel_carve_text(res)))
    assert all(res[k] > 0 for k in STATS) and "carved 0" not in events[1]
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("".join("%r %r %r\n" % tuple(float(v) for v in row) for row in xyyaw))
    out = str(tmp_path / "drive.ply")
    capsys.readouterr()
    sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt"), "--voxel-map", out,
             "--voxel-carve", "15,2,64"])
    said = [line for line in capsys.readouterr().out.splitlines() if line.startswith("voxel map carved")]
    assert said == events
    want = _host(world.rows())
    head, payload = _read_ply(out)
    rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert head[2] == "element vertex %d" % want["count"] and want["count"] > 1000
    assert np.array_equal(rec["xyz"].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(rec["rgb"], want["color"][:, 2::-1])
