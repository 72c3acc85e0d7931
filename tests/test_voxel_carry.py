"""A voxel map carried into another (group (S)): stereo_vision.sv.voxel_map_carry / voxel_map_shifted / voxel_map_recenter_shift against
the per-voxel model of voxel_carry_cases, and engine.voxel_map_carry / rig.VoxelMap.prune, .recenter, .resize, .merge / the CLI against the
definition.  Every comparison is shape, dtype and bits."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
import voxel_carry_cases as carry
import voxel_map_cases as cases
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_carry_cases import STATS
from voxel_map_cases import BOX16, FIELDS, PROBE_BOX

SV_ERR_ARG = -1
SWEEP_BOXES = ((-51.2, 51.2, 0.1), (-40.0, 40.0, 0.05), (-3.0, 5.0, 0.2), (-25.6, 25.6, 0.4), (0.3, 12.7, 0.1))


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


def _summary(sv, state):
    """What a map is compared by: its rows in f64, and (claimed, dropped, overflowed)."""
    return sv.voxel_map_rows(state, dtype="f64"), (len(state["key"]), state["dropped"], state["overflowed"])


def _numpy_carry(sv, case):
    dst, src = _define(sv, *case["dst"]), _define(sv, *case["src"])
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in src.items()}
    stats = sv.voxel_map_carry(dst, src, **case["kw"])
    assert all(np.array_equal(src[k], before[k]) if isinstance(before[k], np.ndarray) else src[k] == before[k] for k in before)  # src is only read
    return _summary(sv, dst) + ([stats[k] for k in STATS],)


@pytest.fixture(scope="module")
def all_cases(sv):
    return dict(carry.carry_cases(sv.voxel_map_slot_of), **carry.gpu_cases(sv.voxel_map_slot_of))


@pytest.fixture(scope="module")
def defined(sv, all_cases):
    """The numpy form's result per case, computed once and shared by the CPU and the GPU tests."""
    return {name: _numpy_carry(sv, case) for name, case in all_cases.items()}


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_the_numpy_form_against_the_model(sv, all_cases, defined):
    for name, case in all_cases.items():
        dst, src = carry.model_map(*case["dst"]), carry.model_map(*case["src"])
        stats = carry.model_carry(dst, src, **case["kw"])
        want = carry.model_rows(dst)
        rows, (claimed, dropped, overflowed), counts = defined[name]
        assert _same(rows, want), name
        assert (claimed, dropped, overflowed) == (want["claimed"], want["dropped"], want["overflowed"]), name
        assert counts == [stats[k] for k in STATS], name


def test_hand_case(sv, defined):
    rows, head, counts = defined["hand"]
    # src: (1,1,1) n 8 m 2 | (2,2,2) n 1: filtered by min_n = 2 | (15,3,3): x + 1 = 16 leaves the box | (4,4,4) n 8 m 2; one row of src dropped
    assert counts == [2, 1, 1, 1] and head == (4, 1, False)
    assert rows["cell"].tolist() == [[0, 0, 0], [2, 2, 2], [5, 5, 5], [9, 9, 9]] and rows["count"] == 4
    assert rows["n"].tolist() == [1, 12, 8, 6] and rows["m"].tolist() == [1, 3, 2, 1]
    assert rows["first_seq"].tolist() == [0, 0, 1, 1] and rows["last_seq"].tolist() == [0, 1, 2, 1]
    # S of (2,2,2): 4 * 32768 of dst + (3 * 16384 + 5 * 49152) of src = 425984; of (5,5,5): 7 * 49152 + 32768 = 376832
    assert rows["xyz"][1].tolist() == [2.0 + (425984 + 6.0) / (65536.0 * 12)] * 3 and rows["xyz"][2].tolist() == [5.0 + (376832 + 4.0) / (65536.0 * 8)] * 3
    # C of (2,2,2): 400 each + (280, 360, 440, 520) -> (2 C + 12) // 24; of (5,5,5): (350, 420, 490, 815) -> (2 C + 8) // 16
    assert rows["color"].tolist() == [[0, 0, 0, 0], [57, 63, 70, 77], [44, 53, 61, 102], [100, 100, 100, 100]]


def test_what_the_cases_cover(sv, defined):
    assert [defined["filter_min_n_%d" % v][2][:2] for v in (4, 5, 6, 7)] == [[3, 3], [2, 4], [1, 5], [0, 6]]
    assert [defined["filter_min_rows_%d" % v][2][:2] for v in (0, 1, 2, 3)] == [[6, 0], [6, 0], [3, 3], [1, 5]]
    assert [defined["filter_since_%d" % v][2][:2] for v in (0, 1, 2, 3)] == [[6, 0], [3, 3], [2, 4], [0, 6]]
    assert defined["shift_16_0_0"][2] == [0, 0, 20, 0] and defined["shift_0_0_-16"][2] == [0, 0, 20, 0] and defined["shift_-1_0_0"][2] == [16, 0, 4, 16]
    assert defined["merge"][2] == [4, 0, 0, 1] and defined["dropped"][1][1] == 3
    assert defined["overflowed_source"][2] == [-1, 0, 0, 0] and defined["overflowed_source"][1] == (3, 1, True) and defined["overflowed_source"][0]["count"] == -1
    assert defined["overflowed_destination"][2] == [-1, 0, 0, 0] and defined["overflowed_destination"][1] == (3, 1, True)
    assert defined["capacity_exactly"][1] == (512, 0, False) and defined["capacity_one_above"][1] == (512, 0, True)
    assert defined["capacity_one_above_merge"][1] == (301, 0, True) and defined["capacity_one_above_merge"][2] == [202, 0, 0, 201]
    assert int(defined["wide_words"][0]["n"][0]) == 512 * (2 ** 31 - 1) > 2 ** 32 and int(defined["wide_words_merge"][0]["n"][0]) == 1024 * (2 ** 31 - 1)
    assert defined["shrink"][2][1] > 0 and defined["grow"][2][0] == 500


def test_a_copy_equals_the_source_field_by_field(sv, all_cases):
    case = all_cases["copy"]
    src, dst = _define(sv, *case["src"]), _define(sv, *case["dst"])
    stats = sv.voxel_map_carry(dst, src)
    assert stats == {"carried": len(src["key"]), "filtered": 0, "outside": 0, "claimed": len(src["key"])}
    for f in ("key", "n", "S", "C", "m", "first_seq", "last_seq"):
        assert dst[f].dtype == src[f].dtype and np.array_equal(dst[f], src[f]), f
    assert (dst["dropped"], dst["overflowed"]) == (src["dropped"], src["overflowed"])


def test_there_and_back_restores_the_map(sv):
    rng = np.random.default_rng(3)
    cells = rng.integers(3, 12, (200, 3))
    src = _define(sv, BOX16, [carry.frames([cells[:120], cells[80:]], weights=(1, 9), seed=1)])
    k = (3, -2, 4)
    there, back = sv.voxel_map_state(src["params"]), sv.voxel_map_state(src["params"])
    a = sv.voxel_map_carry(there, src, shift=k)
    b = sv.voxel_map_carry(back, there, shift=tuple(-v for v in k))
    assert a == b and a["outside"] == 0 and a["carried"] == len(src["key"])
    assert not np.array_equal(there["key"], src["key"])
    for f in ("key", "n", "S", "C", "m", "first_seq", "last_seq"):
        assert np.array_equal(back[f], src[f]), f


def test_a_shifted_box_keeps_its_cells(sv):
    tried = 0
    for lo, hi, size in SWEEP_BOXES:
        params = sv.voxel_map_params((lo,) * 3, (hi,) * 3, size, 512)
        for k in range(-2000, 2001, 7):
            moved = sv.voxel_map_shifted(params, (k, -k, k // 3))
            assert moved["cells"] == params["cells"] and moved["size"] == params["size"] and moved["capacity"] == 512
            assert moved["lo"] == (lo + k * size, lo + -k * size, lo + (k // 3) * size)
            assert sv.voxel_map_params(moved["lo"], moved["hi"], moved["size"], 512) == moved  # what the C entry recomputes
            tried += 1
    assert tried == 5 * 572
    params = sv.voxel_map_params((0.0,) * 3, (1.0,) * 3, 1.0, 512)
    assert sv.voxel_map_shifted(params, (0, 0, 0)) == params and sv.voxel_map_shifted(params, (1, 2, 3), capacity=4096)["capacity"] == 4096
    for bad in ((1, 2), (1, 2, 0.5), (1, 2, 2 ** 31), (True, 0, 0), 5, (1, 2, "x")):
        with pytest.raises(ValueError):
            sv.voxel_map_shifted(params, bad)
    far = sv.voxel_map_params((2.0 ** 53 - 1,) * 3, (2.0 ** 53 + 6,) * 3, 0.5, 512)  # 14 cells, and beyond 2^53 the doubles are 2 apart:
    assert far["cells"] == (14, 14, 14)
    with pytest.raises(ValueError):  # moved by a cell the box can only have 12 or 16 of them
        sv.voxel_map_shifted(far, (2, 0, 0))


def test_the_recenter_shift(sv):
    params = sv.voxel_map_params((-51.2, -51.2, -2.0), (51.2, 51.2, 2.0), 0.1, 512)
    assert params["cells"] == (1024, 1024, 40)
    assert sv.voxel_map_recenter_shift(params, 0.0, 0.0, 0.0) == (0, 0, 0) and sv.voxel_map_recenter_shift(params, 0.0, 0.0) == (0, 0, 0)
    assert sv.voxel_map_recenter_shift(params, 10.05, -3.0) == (100, -30, 0) and sv.voxel_map_recenter_shift(params, 0.0, 0.0, 1.05) == (0, 0, 10)
    for x, y, z in ((12.34, -56.78, 0.3), (-400.0, 250.0, None), (0.049, 0.051, -1.99)):
        k = sv.voxel_map_recenter_shift(params, x, y, z)
        moved = sv.voxel_map_shifted(params, k)
        for a, p in enumerate((x, y, z)):
            if p is not None:  # the point lies in the middle cell of the moved box, up to the rounding of lo'
                assert abs((p - moved["lo"][a]) / 0.1 - (params["cells"][a] // 2 + 0.5)) <= 0.5 + 1e-9
        assert max(abs(v) for v in sv.voxel_map_recenter_shift(moved, x, y, z)) <= 1  # 0 but for a point on a cell's edge, which the rounding of lo' may cross
    for bad in ((np.nan, 0.0, None), (0.0, np.inf, None), (0.0, 0.0, np.nan), (1e300, 0.0, None), (None, 0.0, None)):
        with pytest.raises(ValueError):
            sv.voxel_map_recenter_shift(params, *bad)


def test_the_position_bound(sv):
    """A carried voxel's position in the moved box against its position before: equal up to the bound voxel_map_shifted derives."""
    rng = np.random.default_rng(9)
    params = sv.voxel_map_params((-51.2,) * 3, (51.2,) * 3, 0.1, 4096)
    pts = rng.uniform(-10.0, 10.0, (1, 3000, 3))  # cells 412 .. 612: a shift of up to 400 cells keeps them in the box
    src = sv.voxel_map_state(params)
    sv.voxel_map_insert(src, pts, None, rng.integers(1, 99, (1, 3000)).astype(np.int32), np.array([3000], np.int32), cases.IDENTITY[None])
    before = sv.voxel_map_rows(src, dtype="f64")
    differ = 0
    for k in ((1, -1, 0), (7, 300, -400), (-333, 129, 64), (400, 400, 400)):
        moved = sv.voxel_map_shifted(params, k)
        dst = sv.voxel_map_state(moved)
        stats = sv.voxel_map_carry(dst, src, shift=tuple(-v for v in k))
        assert stats["carried"] == before["count"] and stats["outside"] == 0
        after = sv.voxel_map_rows(dst, dtype="f64")  # in the same order: every key moved by the same cells, none wrapped
        assert np.array_equal(after["cell"], before["cell"] - np.array(k, np.int32)) and np.array_equal(after["n"], before["n"])
        bound = sv.voxel_map_shift_bound(params, moved, k, before["cell"], before["xyz"], after["xyz"])
        assert bound.max() < 1e-13 and (np.abs(after["xyz"] - before["xyz"]) <= bound).all()
        differ += int((after["xyz"] != before["xyz"]).sum())
    assert differ > 0  # and it is a bound on something: the roundings do show


def test_value_errors(sv):
    a, b = sv.voxel_map_state(sv.voxel_map_params(**BOX16)), sv.voxel_map_state(sv.voxel_map_params(**BOX16))
    with pytest.raises(ValueError):
        sv.voxel_map_carry(a, a)
    with pytest.raises(ValueError):
        sv.voxel_map_carry(a, sv.voxel_map_state(sv.voxel_map_params(**dict(BOX16, size=np.nextafter(1.0, 2.0)))))
    for shift in ((0, 0), (0, 0, 0, 0), (2 ** 20 + 1, 0, 0), (0, -2 ** 20 - 1, 0), (0.5, 0, 0), (True, 0, 0), 3, ("a", 0, 0)):
        with pytest.raises(ValueError):
            sv.voxel_map_carry(a, b, shift=shift)
    for kw in (dict(min_n=1.5), dict(min_rows=True), dict(since=0.25)):
        with pytest.raises(ValueError):
            sv.voxel_map_carry(a, b, **kw)
    assert sv.voxel_map_carry(a, b, shift=(2 ** 20, -2 ** 20, 0)) == dict.fromkeys(STATS, 0) and len(a["key"]) == 0


def _cpu_map(params, calls):
    world = util.pkg("rig").VoxelMap(params["lo"], params["hi"], params["size"], params["capacity"], device="cpu")
    for call in calls:
        world.update(*call)
    return world


def test_the_cpu_object_runs_the_definition(sv):
    rng = np.random.default_rng(4)
    box = dict(lo=(-8.0, -8.0, -2.0), hi=(8.0, 8.0, 2.0), size=0.5, capacity=2048)
    call = (rng.uniform(-9, 9, (3, 400, 3)) * [1, 1, 0.25], rng.integers(0, 256, (3, 400, 4)).astype(np.uint8), None, np.array([400, 300, 400], np.int32),
            np.tile(cases.IDENTITY, (3, 1)))
    world, state = _cpu_map(box, [call]), _define(sv, box, [call])
    # prune: the same box, the voxels of the last frame
    want = sv.voxel_map_state(state["params"])
    stats = sv.voxel_map_carry(want, state, since=2)
    assert world.prune(since=2) == stats and stats["filtered"] > 0 and world.seq == 3
    assert _same(_host(world.rows(dtype="f64")), sv.voxel_map_rows(want, dtype="f64"))
    # recenter: nothing to do in the middle cell; then a move
    assert world.recenter(0.1, 0.1) == dict.fromkeys(STATS, 0) and world.params == want["params"]
    with pytest.raises(TypeError):
        world.recenter(0.1, 0.1, min_weight=3)
    k = sv.voxel_map_recenter_shift(world.params, 3.3, -2.2, None)
    assert k == (6, -5, 0)
    moved = sv.voxel_map_state(sv.voxel_map_shifted(want["params"], k))
    stats = sv.voxel_map_carry(moved, want, shift=(-6, 5, 0))
    assert world.recenter(3.3, -2.2) == stats and stats["outside"] > 0 and world.params == moved["params"] and world.params["lo"] == (-5.0, -10.5, -2.0)
    assert world.stats() == {"claimed": len(moved["key"]), "dropped": moved["dropped"], "overflowed": False}
    # resize, and merge with a map whose box starts elsewhere
    stats = world.resize(512)
    assert world.params["capacity"] == 512 and stats["carried"] == len(moved["key"]) and world.stats()["overflowed"] == (len(moved["key"]) > 512)
    other = _cpu_map(box, [call[:3] + (np.array([50, 0, 0], np.int32),) + call[4:], call])
    into = _cpu_map(dict(box, lo=(-5.0, -10.5, -2.0), hi=(11.0, 5.5, 2.0)), [])
    stats = into.merge(other, min_rows=1)
    assert into.seq == 6 and stats["carried"] + stats["outside"] == other.stats()["claimed"] and stats["carried"] == stats["claimed"] > 0
    with pytest.raises(ValueError):
        into.merge(_cpu_map(dict(box, lo=(-5.0, -10.25, -2.0)), []))  # half a cell off
    with pytest.raises(ValueError):
        into.merge(_cpu_map(dict(box, size=0.25), []))
    with pytest.raises(ValueError):
        into.merge(into)
    off = 0.5 / 65536 / 2  # within the tolerance: accepted
    assert into.merge(_cpu_map(dict(box, lo=(-8.0 + off, -8.0, -2.0)), []))["carried"] == 0


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\(?\b(sv_\w*carry\w*)\)?\s*\(", src) == ["sv_voxel_map_carry_device"]
    assert text.index("/* ---- (R)") < text.index("/* ---- (S)") < text.index("/* ---- (A)") and " *  (S) " in text
    assert set(util.pkg("engine").STAGE_SIGNATURES["voxel_carry"]) == {"sv_voxel_map_carry_device"}
    build = util.pkg("build")
    assert "voxel_carry_kernels.hip" in build.SOURCES and "voxel_carry.cpp" in build.SOURCES and "voxel_carry_kernels.h" in build.HEADERS
    assert all(n in sv.__doc__ for n in ("voxel_map_carry", "voxel_map_shifted", "voxel_map_recenter_shift")) and "(S)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_carry_kernels.hip")).read()
    assert "asm" not in source and "atomicAdd(float" not in source
    # slot_of, the claiming probe with its look at the overflow flag, and the filters are the map's own, defined once
    header = cases.check_map_table(build)
    assert source.count("vmap_claim(") == 1 and source.count("vmap_passes(") == 1
    for line in ("if (old != VMAP_EMPTY && old != key) continue;", "if ((probe & 15) == 15 && vmap_overflowed_meanwhile(head)) break;"):
        assert cases.squeeze(line) in header and cases.squeeze(line) not in cases.squeeze(source), line


def test_cli_argument_errors(sv, tmp_path):
    poses, ply, out = str(tmp_path / "poses.txt"), str(tmp_path / "ply"), str(tmp_path / "drive.ply")
    with open(poses, "w") as f:
        f.write("0 0 0\n")
    for bad in (["--voxel-window"], ["--voxel-forget", "3"], ["--batch", "2", "--ply", ply, "--voxel", "0.2", "--voxel-window"],
                ["--batch", "2", "--ply", ply, "--voxel", "0.2", "--poses", poses, "--voxel-map", out, "--voxel-forget", "-1"]):
        with pytest.raises(SystemExit):
            sv.main(["-k", str(tmp_path / "kitti")] + bad)
    assert not os.path.exists(out) and not os.path.exists(ply)


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


def _engine_carry(eng, sv, case):
    import torch
    (dbuf, dwords), (sbuf, swords) = _engine_map(eng, sv, *case["dst"]), _engine_map(eng, sv, *case["src"])
    before = sbuf.clone()
    stats = eng.voxel_map_carry(dbuf, dwords, sbuf, swords, **case["kw"])
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (4,) and stats.device == dbuf.device
    rows = _host(eng.voxel_map_rows(dbuf, dwords, dtype="f64"))
    assert torch.equal(sbuf, before)  # src is only read
    return rows, eng.voxel_map_stats(dbuf), stats.cpu().tolist()


@pytest.mark.gpu
def test_the_device_against_the_numpy_form(sv, eng, all_cases, defined):
    for name, case in all_cases.items():
        rows, head, counts = _engine_carry(eng, sv, case)
        want_rows, want_head, want_counts = defined[name]
        assert _same(rows, want_rows), name
        assert head == want_head, (name, head, want_head)
        assert counts == want_counts, (name, counts, want_counts)


@pytest.mark.gpu
def test_the_destination_table_wraps(sv, eng, all_cases):
    """The probe-wrap cases are what they claim: the chain of the destination runs over the table's end."""
    dbuf, dwords = _engine_map(eng, sv, *all_cases["probe_wrap_empty_1023"]["dst"])
    sbuf, swords = _engine_map(eng, sv, *all_cases["probe_wrap_empty_1023"]["src"])
    eng.voxel_map_carry(dbuf, dwords, sbuf, swords)
    table = dbuf[4:4 + 11 * 1024].view(1024, 11)[:, 0].cpu().numpy()
    assert (table[:11] != -1).all() and table[11] == -1 and table[1023] != -1 and (table[12:1023] == -1).all()


@pytest.mark.gpu
def test_carry_twice_and_a_chain_of_carries(sv, eng, all_cases):
    """The counts are written by every call whatever the tensor held, and a carried map carries on: src -> a -> b, against the numpy form."""
    case = all_cases["merge_shifted_filtered"]
    sbuf, swords = _engine_map(eng, sv, *case["src"])
    src = _define(sv, *case["src"])
    abuf, awords = _engine_map(eng, sv, PROBE_BOX, [])
    bbuf, bwords = _engine_map(eng, sv, dict(BOX16, capacity=4096), [])
    a, b = sv.voxel_map_state(awords), sv.voxel_map_state(bwords)
    for _ in range(2):  # the second time every voxel is found, none claimed
        got = eng.voxel_map_carry(abuf, awords, sbuf, swords, shift=(40, 0, 5)).cpu().tolist()
        want = sv.voxel_map_carry(a, src, shift=(40, 0, 5))
        assert got == [want[k] for k in STATS]
    assert got[3] == 0 and got[0] > 0
    got = eng.voxel_map_carry(bbuf, bwords, abuf, awords, shift=(-38, 12, -5), min_n=2).cpu().tolist()
    want = sv.voxel_map_carry(b, a, shift=(-38, 12, -5), min_n=2)
    assert got == [want[k] for k in STATS] and got[2] > 0
    assert _same(_host(eng.voxel_map_rows(bbuf, bwords, dtype="f64")), sv.voxel_map_rows(b, dtype="f64"))
    assert _same(_host(eng.voxel_map_rows(abuf, awords)), sv.voxel_map_rows(a)) and eng.voxel_map_stats(bbuf) == (len(b["key"]), b["dropped"], False)


@pytest.mark.gpu
def test_match_against_a_map_and_its_copy(sv, eng, all_cases):
    case = all_cases["grow"]
    sbuf, swords = _engine_map(eng, sv, *case["src"])
    dbuf, dwords = _engine_map(eng, sv, *case["dst"])
    eng.voxel_map_carry(dbuf, dwords, sbuf, swords)
    xyz, _, n, counts, _ = case["src"][1][0]
    poses = sv.voxel_map_pose(*np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.3, -0.2, 0.05), (-1.0, 2.0, 0.0)]).T)
    poses = np.tile(poses[None], (xyz.shape[0], 1, 1))
    args = (_cuda(xyz.astype(np.float32)), _cuda(n), _cuda(counts), poses)
    one, two = eng.voxel_map_match(sbuf, swords, *args, min_rows=1), eng.voxel_map_match(dbuf, dwords, *args, min_rows=1)
    for f in one.__slots__:
        assert np.array_equal(getattr(one, f).cpu().numpy(), getattr(two, f).cpu().numpy()), f
    assert int(one.hits.sum()) > 0


def _rig_pair(box, calls):
    rigmod = util.pkg("rig")
    pair = [rigmod.VoxelMap(box["lo"], box["hi"], box["size"], box["capacity"], device=d) for d in ("cuda", "cpu")]
    for call in calls:
        pair[0].update(*(None if a is None else _cuda(a) for a in call[:4]), call[4])
        pair[1].update(*call)
    return pair


def _agree(gpu, cpu, stats=None):
    """The two objects hold the same map; stats = (the device's tensor, the CPU's dict) of the call that led here."""
    assert gpu.params == cpu.params and gpu.seq == cpu.seq and gpu.stats() == cpu.stats()
    assert _same(_host(gpu.rows(dtype="f64")), _host(cpu.rows(dtype="f64")))
    if stats is not None:
        assert stats[0].cpu().tolist() == [stats[1][k] for k in STATS], (stats[0].cpu().tolist(), stats[1])


@pytest.mark.gpu
def test_the_methods_of_the_map_on_both_devices(sv, eng):
    box = dict(lo=(-8.0, -8.0, -2.0), hi=(8.0, 8.0, 2.0), size=0.5, capacity=2048)

    def call(seed, at=(0.0, 0.0)):
        r = np.random.default_rng(seed)
        xyz = (r.uniform(-9, 9, (2, 500, 3)) * [1, 1, 0.25] + [at[0], at[1], 0.0]).astype(np.float32)
        return (xyz, r.integers(0, 256, (2, 500, 4)).astype(np.uint8), r.integers(1, 9, (2, 500)).astype(np.int32), np.array([500, 321], np.int32),
                np.tile(cases.IDENTITY, (2, 1)))

    gpu, cpu = _rig_pair(box, [call(1), call(2)])
    _agree(gpu, cpu)
    first = gpu.buffer.data_ptr()
    _agree(gpu, cpu, (gpu.prune(min_n=4, since=1), cpu.prune(min_n=4, since=1)))
    spare = gpu.buffer.data_ptr()
    assert spare != first and gpu._spare.data_ptr() == first
    zeros = gpu.recenter(0.2, 0.2)
    assert zeros.cpu().tolist() == [0, 0, 0, 0] and gpu.buffer.data_ptr() == spare and cpu.recenter(0.2, 0.2) == dict.fromkeys(STATS, 0)
    _agree(gpu, cpu, (gpu.recenter(3.3, -2.2), cpu.recenter(3.3, -2.2)))  # twice in a row: the buffers swap back
    assert gpu.buffer.data_ptr() == first and gpu.params["lo"] == (-5.0, -10.5, -2.0)
    _agree(gpu, cpu, (gpu.recenter(5.1, -2.2, 0.6, min_rows=1), cpu.recenter(5.1, -2.2, 0.6, min_rows=1)))
    assert gpu.buffer.data_ptr() == spare and gpu.params["lo"][2] == -1.5
    # update and match in the moved box
    more = call(3, at=(5.0, -2.0))
    gpu.update(*(_cuda(a) for a in more[:4]), more[4])
    cpu.update(*more)
    _agree(gpu, cpu)
    poses = np.tile(sv.voxel_map_pose(*np.array([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0), (0.1, -0.1, 0.02)]).T)[None], (2, 1, 1))
    one, two = gpu.match(_cuda(more[0]), _cuda(more[2]), _cuda(more[3]), poses), cpu.match(more[0], more[2], more[3], poses)
    for f in one.__slots__:
        assert np.array_equal(getattr(one, f).cpu().numpy(), getattr(two, f).numpy()), f
    assert int(one.hits[:, 0].sum()) > 0
    # resize: smaller than what it holds overflows, as on the CPU; larger keeps everything; the spare follows on the next use
    held = gpu.stats()["claimed"]
    _agree(gpu, cpu, (gpu.resize(4096), cpu.resize(4096)))
    assert gpu.params["capacity"] == 4096 and gpu._spare is None and gpu.stats()["claimed"] == held and gpu.buffer.numel() * 8 == eng.voxel_map_lib().sv_voxel_map_bytes(4096)
    _agree(gpu, cpu, (gpu.prune(min_rows=1), cpu.prune(min_rows=1)))
    assert gpu._spare.numel() == gpu.buffer.numel()
    # merge: another map whose box starts 4 x 3 x 0 cells away
    other = _rig_pair(dict(box, lo=(-3.0, -9.0, -1.5), hi=(13.0, 7.0, 2.5)), [call(4, at=(5.0, -2.0)), call(5), call(6)])
    _agree(gpu, cpu, (gpu.merge(other[0], min_n=2), cpu.merge(other[1], min_n=2)))
    assert gpu.seq == 6 and _same(_host(other[0].rows()), _host(other[1].rows()))
    small = _rig_pair(dict(gpu.params, capacity=512), [])
    got, want = small[0].merge(gpu), small[1].merge(cpu)  # more than it can hold: it overflows during the call, and `claimed` means nothing then
    assert got.cpu().tolist()[:3] == [want[k] for k in STATS[:3]] and want["carried"] > 512
    assert small[0].stats()["overflowed"] and small[1].stats()["overflowed"] and small[0].rows()["count"] == small[1].rows()["count"] == -1
    got, want = small[0].prune(), small[1].prune()  # an overflowed map stays lost: carried -1
    assert got.cpu().tolist() == [want[k] for k in STATS] == [-1, 0, 0, 0] and small[0].stats()["overflowed"] and small[0].rows()["count"] == -1
    with pytest.raises(ValueError):
        gpu.merge(cpu)


def _spec(eng, sv, params):
    return eng.voxel_map_spec(sv.voxel_map_params(**params))


@pytest.mark.gpu
def test_the_c_entry_refuses(sv, eng, all_cases):
    import torch
    L = eng.voxel_carry_lib()
    case = all_cases["merge"]
    (dbuf, dwords), (sbuf, swords) = _engine_map(eng, sv, *case["dst"]), _engine_map(eng, sv, *case["src"])
    big = torch.zeros(dbuf.numel() * 2 + 8, dtype=torch.int64, device="cuda")
    stats = torch.full((6,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    keep = [t.clone() for t in (dbuf, sbuf, stats)]
    need = dbuf.numel() * 8
    good = dict(dst=dbuf.data_ptr(), dst_bytes=need, dst_spec=_spec(eng, sv, BOX16), src=sbuf.data_ptr(), src_bytes=need, src_spec=_spec(eng, sv, BOX16),
                shift=(0, 0, 0), stats=stats.data_ptr())

    def call(**change):
        a = dict(good, **change)
        spec = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731
        return L.sv_voxel_map_carry_device(a["dst"], a["dst_bytes"], spec(a["dst_spec"]), a["src"], a["src_bytes"], spec(a["src_spec"]), *a["shift"], 1, 1, 0, a["stats"],
                                           torch.cuda.current_stream().cuda_stream)

    def spec_with(**words):
        s = _spec(eng, sv, BOX16)
        for k, v in words.items():
            if k in ("lo", "hi"):
                getattr(s, k)[0] = v
            elif k == "reserved":
                s.reserved[3] = v
            else:
                setattr(s, k, v)
        return s

    bad = []
    for which in ("dst", "src"):
        bad += [{which + "_spec": None}, {which: None}, {which: good[which] + 8}, {which + "_bytes": need - 8}, {which + "_bytes": 0}]
        bad += [{which + "_spec": spec_with(**w)} for w in (dict(reserved=1), dict(size=0.0), dict(size=float("nan")), dict(size=float("inf")), dict(lo=float("-inf")),
                                                            dict(hi=float("nan")), dict(lo=16.0), dict(size=1e-6), dict(capacity=0), dict(capacity=2 ** 26 + 1))]
    bad += [{"src_spec": spec_with(size=float(np.nextafter(1.0, 2.0)))}, {"dst_spec": spec_with(size=0.5)}]
    bad += [{"shift": s} for s in ((2 ** 20 + 1, 0, 0), (0, -2 ** 20 - 1, 0), (0, 0, 2 ** 20 + 1), (-2 ** 31, 0, 0))]
    bad += [{"src": good["dst"]}, {"dst": big.data_ptr(), "dst_bytes": big.numel() * 8, "src": big.data_ptr() + need}, {"dst": big.data_ptr() + 16, "src": big.data_ptr(), "src_bytes": need + 16},
            {"src": big.data_ptr(), "src_bytes": big.numel() * 8, "dst": big.data_ptr() + need + 16}]
    bad += [{"stats": good["stats"] + 4}, {"stats": good["dst"] + 64}, {"stats": good["src"] + need - 8}, {"stats": good["src"]}]
    for change in bad:
        eng.lib().sv_last_error(None)
        assert call(**change) == SV_ERR_ARG, change
        text = eng.lib().sv_last_error(None)
        assert text and b"sv_voxel_map_carry" in text, change
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((dbuf, sbuf, stats), keep)) and not big.any().item()
    # and the same call, unchanged, is taken: with stats, and with none
    dst, src = _define(sv, *case["dst"]), _define(sv, *case["src"])
    want = sv.voxel_map_carry(dst, src)
    assert call() == 0
    assert stats.cpu().tolist() == [want[k] for k in STATS] + [7, 7]
    assert _same(_host(eng.voxel_map_rows(dbuf, dwords, dtype="f64")), sv.voxel_map_rows(dst, dtype="f64"))
    sv.voxel_map_carry(dst, src, shift=(1, 0, 0))
    assert call(stats=None, shift=(1, 0, 0)) == 0
    assert _same(_host(eng.voxel_map_rows(dbuf, dwords, dtype="f64")), sv.voxel_map_rows(dst, dtype="f64")) and stats.cpu().tolist()[4:] == [7, 7]
    assert eng.voxel_map_stats(dbuf) == (len(dst["key"]), dst["dropped"], False)
    # the wrapper's own checks
    for kw in (dict(shift=(0, 0)), dict(shift=(2 ** 20 + 1, 0, 0)), dict(shift=(0.5, 0, 0)), dict(min_n=0.5), dict(since=2 ** 31)):
        with pytest.raises(ValueError):
            eng.voxel_map_carry(dbuf, dwords, sbuf, swords, **kw)
    with pytest.raises(ValueError):
        eng.voxel_map_carry(dbuf, dwords, dbuf, dwords)
    with pytest.raises(ValueError):
        eng.voxel_map_carry(dbuf, dwords, sbuf, dict(swords, size=0.5))


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    at = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:at].decode().splitlines(), data[at:]


@pytest.mark.gpu
def test_cli_window_and_forget(sv, eng, tmp_path, capsys):
    """--voxel-window and --voxel-forget over two batches against the same sequence driven through the CPU object, and the command without
    them against a map driven by hand."""
    from PIL import Image
    from test_occupancy_map import H, W, _drive_frames
    n = 4
    ls, rs = _drive_frames(n)
    xyyaw = np.array([[0.0, 0.0, 0.0], [0.8, 0.05, 0.03], [120.0, -1.0, 0.06], [120.8, -1.0, 0.09]])  # either batch starts outside the middle third
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
    plain = rigmod.VoxelMap(lo, hi, 0.2, sv.CLI_VOXEL_MAP_CAPACITY, device="cpu")
    events = []
    for i in (0, 2):
        if sv.cli_voxel_window_left(world.params, xyyaw[i, 0], xyyaw[i, 1]):
            events.append("voxel map recentred at frame %d: %s" % (i, sv.cli_voxel_carry_text(world.recenter(xyyaw[i, 0], xyyaw[i, 1]))))
        for m in (world, plain):
            m.update(xyz[i:i + 2], color[i:i + 2], cnt[i:i + 2], counts[i:i + 2], poses[i:i + 2])
        events.append("voxel map pruned after frame %d: %s" % (i + 1, sv.cli_voxel_carry_text(world.prune(since=world.seq - 2))))
    assert len(events) == 4 and events[0] == "voxel map recentred at frame 0: carried 0, filtered 0, outside 0, claimed 0"  # an empty map moves too
    assert "recentred at frame 2" in events[2] and " outside 0" not in events[2] and " carried 0" not in events[2] and world.params["lo"] != plain.params["lo"]
    assert "after frame 1" in events[1] and " filtered 0" in events[1] and "after frame 3" in events[3] and " filtered 0" not in events[3]
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("".join("%r %r %r\n" % tuple(float(v) for v in row) for row in xyyaw))
    base = ["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt")]
    for flags, model, printed in ((["--voxel-window", "--voxel-forget", "2"], world, events), ([], plain, [])):
        out = str(tmp_path / ("drive%d.ply" % len(flags)))
        capsys.readouterr()
        sv.main(base + ["--voxel-map", out] + flags)
        said = [line for line in capsys.readouterr().out.splitlines() if line.startswith("voxel map re") or line.startswith("voxel map pruned")]
        assert said == printed
        want = _host(model.rows())
        head, payload = _read_ply(out)
        rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
        assert head[2] == "element vertex %d" % want["count"] and want["count"] > 1000
        assert np.array_equal(rec["xyz"].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(rec["rgb"], want["color"][:, 2::-1])
