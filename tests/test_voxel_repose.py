"""A voxel map re-posed after a loop closure (group (AD)): stereo_vision.sv.voxel_map_repose against its plain loop, the host helpers
pose_corrections and loop_spread against what they promise, one drive with a loop on numpy maps, and engine.voxel_map_repose /
rig.VoxelMap.repose, .merge(pose=...) / rig.PlaceIndex.repose against the definition.  Every comparison of maps is bits."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
import voxel_map_cases as cases
import voxel_repose_cases as repose
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_repose_cases import BOX, STATS

SV_ERR_ARG = -1
WORDS = ("key", "n", "S", "C", "m", "first_seq", "last_seq")


def _define(sv, params, calls, seq=0):
    state = sv.voxel_map_state(sv.voxel_map_params(**params))
    for call in calls:
        sv.voxel_map_insert(state, *call, seq0=seq)
        seq += call[0].shape[0]
    return state


def _pair(sv, case):
    """(dst, src) of a case as numpy maps, src carved where the case says so."""
    dst, src = _define(sv, *case["dst"]), _define(sv, *case["src"], seq=case.get("src_seq0", 0))
    if "carve" in case:
        sv.voxel_map_carve(src, *case["carve"]["frames"], **case["carve"]["kw"])
    return dst, src


def _copy(state):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}


def _same_state(a, b):
    return all(a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and np.array_equal(a[f], b[f]) for f in WORDS) and \
        (a["dropped"], a["overflowed"]) == (b["dropped"], b["overflowed"])


@pytest.fixture(scope="module")
def all_cases():
    return repose.repose_cases()


@pytest.fixture(scope="module")
def defined(sv, all_cases):
    """The numpy form's result per case - (dst afterwards, the counts) -, computed once and shared by the CPU and the GPU tests."""
    out = {}
    for name, case in all_cases.items():
        dst, src = _pair(sv, case)
        before = _copy(src)
        stats = sv.voxel_map_repose(dst, src, case["corr"], **case["kw"])
        assert _same_state(src, before), name  # src is only read
        out[name] = (dst, [stats[k] for k in STATS])
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_the_numpy_form_against_the_plain_loop(sv, all_cases, defined):
    for name, case in all_cases.items():
        dst, src = _pair(sv, case)
        stats = sv.voxel_map_repose_brute(dst, src, case["corr"], **case["kw"])
        assert _same_state(dst, defined[name][0]), name
        assert [stats[k] for k in STATS] == defined[name][1], name


def test_what_the_cases_cover(sv, all_cases, defined):
    count = lambda name: defined[name][1]  # noqa: E731
    voxels = len(_define(sv, *all_cases["frames_8"]["src"])["key"])
    assert 1900 < voxels < 2200 and count("frames_8")[0] + count("frames_8")[2] == voxels and count("frames_8")[3] < count("frames_8")[0]  # many to one
    assert count("one_cell") == [voxels, 0, 0, 1] and count("four_cells") == [voxels, 0, 0, 4] and count("one_cell_held") == [voxels, 0, 0, 0]
    one = defined["one_cell"][0]
    assert len(one["key"]) == 1 and int(one["n"][0]) == int(_define(sv, *all_cases["frames_8"]["src"])["n"].sum()) and (one["first_seq"][0], one["last_seq"][0]) == (0, 7)
    assert count("identity") == [voxels, 0, 0, voxels]
    for name in ("filter_min_n", "filter_min_rows", "filter_since", "filters_together"):
        assert count(name)[1] > 100 and count(name)[0] > 100, name
    # the tombstones are filtered at min_n = 1 and at min_n = 0 alike
    src = _pair(sv, all_cases["tombstones_min_n_0"])[1]
    assert int((src["n"] == 0).sum()) == 10 and count("tombstones_min_n_0") == count("tombstones_min_n_1") == [7, 10, 0, 7]
    # frames 2, 5 and 6 carry a NaN, an inf and a -inf: their voxels are outside, the others' as under the finite corrections
    last = _define(sv, *all_cases["frames_8"]["src"])["last_seq"]
    assert count("not_finite")[2] >= int(np.isin(last, (2, 5, 6)).sum()) > 500 and count("taken_outside")[2] >= int(np.isin(last, (1, 4, 7)).sum()) > 500
    assert count("overflowed_source") == count("overflowed_destination") == [-1, 0, 0, 0]
    assert defined["overflowed_source"][0]["overflowed"] and defined["overflowed_destination"][0]["overflowed"] and defined["overflows_meanwhile"][0]["overflowed"]
    assert count("overflows_meanwhile")[:3] == count("frames_8")[:3]
    # the clamps: with seq0 = 3 and K = 3 the frames 0 .. 3 take corr[0], frame 4 corr[1], frames 5 .. 7 corr[2]
    case = all_cases["index_clamps"]
    dst, src = _pair(sv, case)
    same = sv.voxel_map_repose(dst, src, case["corr"][[0, 0, 0, 0, 1, 2, 2, 2]])
    assert _same_state(dst, defined["index_clamps"][0]) and [same[k] for k in STATS] == count("index_clamps")
    case = all_cases["index_seq_top"]  # last_seq = 2^31 - 9 .. 2^31 - 2 against seq0 = 2^31 - 7: -2 .. 5 clamped into 0 .. 4
    dst, src = _pair(sv, case)
    assert int(src["last_seq"].max()) == 2 ** 31 - 2
    sv.voxel_map_repose(dst, _define(sv, *case["src"]), case["corr"][[0, 0, 0, 1, 2, 3, 4, 4]])
    moved = defined["index_seq_top"][0]
    assert all(np.array_equal(dst[f], moved[f]) for f in ("key", "n", "S", "C", "m")) and np.array_equal(dst["last_seq"] + (2 ** 31 - 9), moved["last_seq"])


def test_an_identity_repose_keeps_the_means_to_a_step(sv, all_cases, defined):
    """No shortcut: S becomes n times a whole offset - floor(S / n + 1 / 2), the centre's, but for a rounding of the doubles on the way -,
    every other word stays, and no centre moves by more than 1 / 65536 of a cell."""
    src = _define(sv, *all_cases["identity"]["src"])
    dst = defined["identity"][0]
    assert all(np.array_equal(dst[f], src[f]) for f in ("key", "n", "C", "m", "first_seq", "last_seq"))
    n = src["n"][:, None]
    u, exact = dst["S"] // n, (2 * src["S"] + n) // (2 * n)
    assert np.array_equal(dst["S"], u * n) and not np.array_equal(dst["S"], src["S"])
    assert np.abs(u - exact).max() <= 1 and (u == exact).mean() > 0.99
    a, b = sv.voxel_map_rows(src, dtype="f64")["xyz"], sv.voxel_map_rows(dst, dtype="f64")["xyz"]
    assert 0 < np.abs(a - b).max() <= BOX["size"] / 65536 * (1 + 1e-9)


def test_the_rounding_edges_are_edges(sv, defined):
    """Every voxel of the rounding case lands where the definition says, and somewhere else under at least one of the three mistakes."""
    case, found = repose.rounding_case()
    src = _define(sv, *case["src"])
    assert len(found) >= 12 and len(src["key"]) == len(found) and all(sum(m in f for f in found) >= 3 for m in repose.MISTAKES)
    want = {}
    for i in range(len(src["key"])):
        key, S, n, last = int(src["key"][i]), src["S"][i].tolist(), int(src["n"][i]), int(src["last_seq"][i])
        w = [float(v) for v in case["corr"][last]]
        right = repose.landing(case["src"][0], case["dst"][0], key, S, n, w)
        moved = [m for m in repose.MISTAKES if repose.landing(case["src"][0], case["dst"][0], key, S, n, w, m) != right]
        assert moved == found[last] and moved, (i, moved, found[last])
        to = sum(c << (20 * k) for k, (c, u) in enumerate(right))
        want.setdefault(to, [0, 0, 0])
        want[to] = [want[to][k] + n * right[k][1] for k in range(3)]
    dst = defined["rounding_edges"][0]
    assert dst["key"].tolist() == sorted(want) and dst["S"].tolist() == [want[k] for k in sorted(want)]


def test_value_errors(sv):
    a, b = sv.voxel_map_state(sv.voxel_map_params(**cases.BOX16)), sv.voxel_map_state(sv.voxel_map_params(**cases.BOX16))
    one = cases.IDENTITY[None]
    for fn in (sv.voxel_map_repose, sv.voxel_map_repose_brute):
        with pytest.raises(ValueError):
            fn(a, a, one)
        for corr in (cases.IDENTITY, np.zeros((0, 12)), np.zeros((2, 11)), np.zeros((1, 1, 12)), "corr", None):
            with pytest.raises(ValueError):
                fn(a, b, corr)
        for kw in (dict(seq0=-1), dict(seq0=2 ** 31 - 1), dict(seq0=0.5), dict(seq0=True), dict(min_n=1.5), dict(min_rows=True), dict(since=0.25)):
            with pytest.raises(ValueError):
                fn(a, b, one, **kw)
        assert fn(a, b, one, seq0=2 ** 31 - 2) == dict.fromkeys(STATS, 0) and len(a["key"]) == 0
    with pytest.raises(ValueError):
        sv.voxel_map_repose(a, b, np.zeros((2 ** 22 + 1, 12)))


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.findall(r"\(?\b(sv_\w*repose\w*)\)?\s*\(", src) == ["sv_voxel_repose_device"]
    assert text.index("/* ---- (AC)") < text.index("/* ---- (AD)") < text.index("/* ---- (A)") and " *  (AD) " in text
    assert set(util.pkg("engine").STAGE_SIGNATURES["voxel_repose"]) == {"sv_voxel_repose_device"}
    build = util.pkg("build")
    assert "voxel_repose_kernels.hip" in build.SOURCES and "voxel_repose.cpp" in build.SOURCES and "voxel_repose_kernels.h" in build.HEADERS
    assert "-ffp-contract=off" in build.COMMON
    assert all(n in sv.__doc__ for n in ("voxel_map_repose", "pose_corrections", "loop_spread")) and "(AD)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_repose_kernels.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert "asm" not in code and "atomicAdd(float" not in code
    # the filters, the centre, the way into a cell and the claiming probe are the map's own, defined once in voxel_map_table.h
    header = cases.check_map_table(build)
    for name in ("vmap_claim(", "vmap_passes(", "vmap_offset("):
        assert code.count(name) == 1, name
    assert code.count("vmap_centre(") == 3 and code.count("vmap_cell(") == 1
    for text in cases.TABLE_TEXTS:
        assert cases.squeeze(text) not in cases.squeeze(source), text
    for line in ("if (old != VMAP_EMPTY && old != key) continue;", "if ((probe & 15) == 15 && vmap_overflowed_meanwhile(head)) break;"):
        assert cases.squeeze(line) in header and cases.squeeze(line) not in cases.squeeze(source), line


# ---------------------------------------------------------------------------------------------------------------- the host helpers

def _mul(sv, a, b):
    return sv._pose_mul(np.asarray(a, np.float64), np.asarray(b, np.float64))


def _close(a, b, bound=1e-9):
    """Two motions agree: the rotations to `bound`, the translations to `bound` relative to their magnitude (at least 1)."""
    a, b = np.asarray(a), np.asarray(b)
    scale = max(1.0, float(np.abs(b[..., 9:]).max()))
    return float(np.abs(a[..., :9] - b[..., :9]).max()) <= bound and float(np.abs(a[..., 9:] - b[..., 9:]).max()) <= bound * scale


def _chain(sv, N=40, seed=5):
    """N true poses of a drive in three dimensions: steps of about a metre that turn slowly about all three axes."""
    rng = np.random.default_rng(seed)
    out = [np.concatenate([np.eye(3).reshape(9), [3.0, -2.0, 0.5]])]
    for _ in range(N - 1):
        out.append(_mul(sv, out[-1], sv.pose_exp(np.concatenate([rng.uniform(-0.05, 0.05, 3), [1.0, 0.0, 0.0] + rng.uniform(-0.1, 0.1, 3)]))))
    return np.array(out)


def test_log_and_exp_are_inverses(sv):
    rng = np.random.default_rng(6)
    for scale in (1e-9, 1e-4, 0.02, 0.5, 2.0, 3.1):
        for _ in range(20):
            om = rng.uniform(-1, 1, 3)
            xi = np.concatenate([om * scale / np.sqrt((om * om).sum()), rng.uniform(-30, 30, 3)])
            E = sv.pose_exp(xi)
            assert np.abs(E[:9].reshape(3, 3) @ E[:9].reshape(3, 3).T - np.eye(3)).max() < 1e-14
            assert np.abs(sv.pose_log(E) - xi).max() <= 1e-9 * 30 and _close(sv.pose_exp(sv.pose_log(E)), E)
    half_turn = sv.pose_exp(np.array([0.0, 0.0, np.pi - 1e-7, 1.0, 2.0, 3.0]))
    with pytest.raises(ValueError):
        sv.pose_log(half_turn)
    assert sv.pose_log(sv.pose_exp(np.array([0.0, 0.0, np.pi - 1e-5, 1.0, 2.0, 3.0])))[2] == pytest.approx(np.pi - 1e-5, abs=1e-9)


def test_pose_corrections(sv):
    old, new = _chain(sv, 12, 1), _chain(sv, 12, 2)
    corr = sv.pose_corrections(old, new)
    assert corr.shape == (12, 12) and corr.dtype == np.float64
    assert all(_close(_mul(sv, corr[k], old[k]), new[k]) for k in range(12))
    assert _close(sv.pose_corrections(old, old), np.tile(cases.IDENTITY, (12, 1)), 1e-12)
    for bad in ((old[:3], new), (old[:, :11], new[:, :11]), (old[0], new[0])):
        with pytest.raises(ValueError):
            sv.pose_corrections(*bad)


def test_loop_spread(sv):
    T = _chain(sv)
    N, i, j = len(T), 6, 31
    xi = np.array([0.01, -0.02, 0.04, 0.8, -1.9, 0.3])  # the drift the loop has gathered at frame j
    weights = np.random.default_rng(8).uniform(0.0, 2.0, j - i)
    weights[3] = 0.0  # a step on which the vehicle stood
    for w in (None, weights):
        f = np.arange(j - i + 1) / (j - i) if w is None else np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
        fk = np.concatenate([np.zeros(i), f, np.ones(N - j - 1)])
        drift = np.array([_mul(sv, T[k], sv.pose_exp(-fk[k] * xi)) for k in range(N)])  # P_k = T_k o exp(-f_k xi) up to frame j
        for k in range(j + 1, N):  # behind the loop the odometry goes on from where it is: the true motions from the drifted frame j
            drift[k] = _mul(sv, drift[j], _mul(sv, sv._pose_inv(T[j]), T[k]))
        got = sv.loop_spread(drift, i, j, T[j], weights=w)
        assert got.shape == (N, 12) and got[:i].tobytes() == drift[:i].tobytes()  # in front of the loop: bit for bit
        assert _close(got[j], T[j])
        assert all(_close(got[k], T[k]) for k in range(N))  # the drift of the spread model is undone
        rel = lambda P, k: _mul(sv, sv._pose_inv(P[k]), P[k + 1])  # noqa: E731
        assert all(_close(rel(got, k), rel(drift, k)) for k in range(j + 1, N - 1))  # behind the loop the motions stay
    # f is monotone in the weights: a step's share of the correction grows with its weight, and is none at weight 0
    E = sv.pose_log(_mul(sv, sv._pose_inv(drift[j]), T[j]))
    share = [np.abs(sv.pose_log(_mul(sv, sv._pose_inv(drift[k]), got[k]))[3:]).max() / np.abs(E[3:]).max() for k in range(i, j + 1)]
    assert all(b >= a - 1e-9 for a, b in zip(share, share[1:])) and share[4] == pytest.approx(share[3], abs=1e-9) and share[-1] == pytest.approx(1.0, abs=1e-9)
    assert sv.loop_spread(drift, i, j, T[j], weights=np.ones(N - 1)).tobytes() == sv.loop_spread(drift, i, j, T[j], weights=np.ones(j - i)).tobytes()
    half_turn = _mul(sv, drift[j], sv.pose_exp(np.array([0.0, 0.0, np.pi - 1e-7, 0.0, 0.0, 0.0])))
    for bad in (dict(i=5, j=5), dict(i=7, j=3), dict(i=-1, j=3), dict(i=0, j=N), dict(i=0.5, j=3), dict(target=half_turn), dict(target=T[:2]),
                dict(weights=-np.ones(j - i)), dict(weights=np.zeros(j - i)), dict(weights=np.ones(j - i + 1)), dict(weights=np.full(j - i, np.nan))):
        with pytest.raises(ValueError):
            sv.loop_spread(drift, **dict(dict(i=i, j=j, target=T[j]), **bad))


def test_pose_repose(sv):
    P, corr = _chain(sv, 6, 3), _chain(sv, 4, 4)
    seq = np.array([0, 9, 10, 11, 12, 40])
    got = sv.pose_repose(P, seq, corr, seq0=9)
    assert all(got[r].tobytes() == _mul(sv, corr[k], P[r]).tobytes() for r, k in enumerate((0, 0, 1, 2, 3, 3)))
    with pytest.raises(ValueError):
        sv.pose_repose(P, seq[:3], corr)


# ---------------------------------------------------------------------------------------------------------------- one drive with a loop

def test_a_loop_closure_repairs_the_map(sv):
    """A wall and three boxes passed twice under poses that drift by the spread model, 1.2 m and more at the second pass: before the
    re-pose 100 % of the second pass's voxels lie in a cell that is neither a cell of the truth map nor 26-adjacent to one; after
    loop_spread, pose_corrections and voxel_map_repose none does."""
    truth = repose.drive_truth(sv)
    N = repose.DRIVE_FRAMES
    xi = np.array([0.0, 0.0, 0.02, 0.3, 2.0, 0.1])
    drift = np.array([sv._pose_mul(truth[k], sv.pose_exp(-(k / (N - 1)) * xi)) for k in range(N)])
    assert min(np.abs(sv.pose_exp(-(k / (N - 1)) * xi)[9:]).max() for k in range(repose.DRIVE_PASS2, N)) >= 4 * repose.DRIVE_BOX["size"]
    xyz, color, n, counts = repose.drive_frames(sv, truth)
    assert 1 < int((counts > 0).sum()) and counts.max() > 500
    true_map = _define(sv, repose.DRIVE_BOX, [(xyz, color, n, counts, truth)])
    drive_map = _define(sv, repose.DRIVE_BOX, [(xyz, color, n, counts, drift)])
    spans = drive_map["last_seq"] - drive_map["first_seq"]
    assert 0 < spans.max() <= 4  # a voxel is seen by a short run of frames
    before, voxels = repose.strangers(drive_map, true_map, repose.DRIVE_PASS2)
    assert voxels > 1000 and before >= 0.25, before
    fixed = sv.loop_spread(drift, 0, N - 1, truth[N - 1])
    moved = sv.voxel_map_state(drive_map["params"])
    stats = sv.voxel_map_repose(moved, drive_map, sv.pose_corrections(drift, fixed))
    assert stats["carried"] == len(drive_map["key"]) and stats["outside"] == stats["filtered"] == 0 and not moved["overflowed"]
    after, voxels = repose.strangers(moved, true_map, repose.DRIVE_PASS2)
    assert voxels > 1000 and after == 0.0, after
    assert repose.strangers(moved, true_map, 0)[0] == 0.0  # and the first pass too
    assert (round(before, 3), after) == (1.0, 0.0)  # the shares DESIGN.md records


# ---------------------------------------------------------------------------------------------------------------- GPU

def _engine_map(eng, sv, params, calls, seq=0):
    words = sv.voxel_map_params(**params)
    buf = eng.voxel_map_new(words)
    for call in calls:
        eng.voxel_map_insert(buf, words, *(None if a is None else _cuda(a) for a in call[:4]), call[4], seq0=seq)
        seq += call[0].shape[0]
    return buf, words


def _table(eng, sv, buf, words):
    """The entries the table of `buf` holds, in ascending key, as the numpy state names them, and (claimed, dropped, overflowed)."""
    slots = sv.voxel_map_slots(words["capacity"])
    t = buf[4:4 + 11 * slots].view(slots, 11).cpu().numpy()
    t = t[t[:, 0] != -1]
    t = t[np.argsort(t[:, 0])]
    return {"key": t[:, 0], "n": t[:, 1], "S": t[:, 2:5], "C": t[:, 5:9], "m": t[:, 9], "first_seq": t[:, 10] & 0xFFFFFFFF, "last_seq": t[:, 10] >> 32}, eng.voxel_map_stats(buf)


def _engine_repose(eng, sv, case):
    import torch
    (dbuf, dwords), (sbuf, swords) = _engine_map(eng, sv, *case["dst"]), _engine_map(eng, sv, *case["src"], seq=case.get("src_seq0", 0))
    if "carve" in case:
        xyz, n, counts, poses = case["carve"]["frames"]
        eng.voxel_map_carve(sbuf, swords, _cuda(xyz), _cuda(n), _cuda(counts), poses, **case["carve"]["kw"])
    before = sbuf.clone()
    stats = eng.voxel_map_repose(dbuf, dwords, sbuf, swords, case["corr"], **case["kw"])
    assert stats.dtype == torch.int64 and tuple(stats.shape) == (4,) and stats.device == dbuf.device
    table, head = _table(eng, sv, dbuf, dwords)
    assert torch.equal(sbuf, before)  # src is only read
    return table, head, stats.cpu().tolist()


@pytest.mark.gpu
def test_the_device_against_the_numpy_form(sv, eng, all_cases, defined):
    for name, case in all_cases.items():
        table, head, counts = _engine_repose(eng, sv, case)
        want, want_counts = defined[name]
        if case.get("loose"):  # dst overflowed during the call: the flag, and the three counts that stay exact
            assert head[2] and want["overflowed"] and head[1] == want["dropped"] and counts[:3] == want_counts[:3], (name, head, counts)
            continue
        for f in WORDS:
            assert table[f].shape == want[f].shape and np.array_equal(table[f], want[f]), (name, f)
        assert head == (len(want["key"]), want["dropped"], want["overflowed"]), (name, head)
        assert counts == want_counts, (name, counts, want_counts)


@pytest.mark.gpu
def test_repose_twice_and_into_a_refused_map(sv, eng, all_cases):
    """The counts are written by every call whatever the tensor held; a second call finds every voxel and claims none; an overflowed map
    on either side leaves the content of dst as it was."""
    case = all_cases["four_cells"]
    (dbuf, dwords), (sbuf, swords) = _engine_map(eng, sv, *case["dst"]), _engine_map(eng, sv, *case["src"])
    dst, src = _pair(sv, case)
    for _ in range(2):
        got = eng.voxel_map_repose(dbuf, dwords, sbuf, swords, case["corr"]).cpu().tolist()
        want = sv.voxel_map_repose(dst, src, case["corr"])
        assert got == [want[k] for k in STATS]
    assert got[3] == 0 and got[0] > 0
    table, head = _table(eng, sv, dbuf, dwords)
    assert all(np.array_equal(table[f], dst[f]) for f in WORDS) and head == (4, 0, False)
    for name in ("overflowed_source", "overflowed_destination"):
        case = all_cases[name]
        (dbuf, dwords), (sbuf, swords) = _engine_map(eng, sv, *case["dst"]), _engine_map(eng, sv, *case["src"])
        before = _table(eng, sv, dbuf, dwords)[0]
        assert eng.voxel_map_repose(dbuf, dwords, sbuf, swords, case["corr"]).cpu().tolist() == [-1, 0, 0, 0]
        after, head = _table(eng, sv, dbuf, dwords)
        assert all(np.array_equal(before[f], after[f]) for f in WORDS) and head[2]


def _host(rows):
    return {k: v if k == "count" else v.cpu().numpy() for k, v in rows.items()}


def _same_rows(got, want):
    for k in cases.FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.tobytes() != b.tobytes():
            return False
    return got["count"] == want["count"]


def _rig_pair(box, calls):
    rigmod = util.pkg("rig")
    pair = [rigmod.VoxelMap(box["lo"], box["hi"], box["size"], box["capacity"], device=d) for d in ("cuda", "cpu")]
    for call in calls:
        pair[0].update(*(None if a is None else _cuda(a) for a in call[:4]), call[4])
        pair[1].update(*call)
    return pair


def _agree(gpu, cpu, stats=None):
    assert gpu.params == cpu.params and gpu.seq == cpu.seq and gpu.stats() == cpu.stats()
    assert _same_rows(_host(gpu.rows(dtype="f64")), _host(cpu.rows(dtype="f64")))
    if stats is not None:
        assert stats[0].cpu().tolist() == [stats[1][k] for k in STATS], (stats[0].cpu().tolist(), stats[1])


@pytest.mark.gpu
def test_the_methods_of_the_map_on_both_devices(sv, eng, all_cases):
    import torch
    case = all_cases["frames_8"]
    gpu, cpu = _rig_pair(BOX, case["src"][1])
    _agree(gpu, cpu)
    first = gpu.buffer.data_ptr()
    gpu.normals(), cpu.normals()
    _agree(gpu, cpu, (gpu.repose(case["corr"]), cpu.repose(case["corr"])))
    assert gpu.buffer.data_ptr() != first and gpu._spare.data_ptr() == first and gpu.seq == 8 and not gpu._normals_fresh and not cpu._normals_fresh
    _agree(gpu, cpu, (gpu.repose(_cuda(case["corr"][:3]), seq0=2, min_n=2, since=1), cpu.repose(torch.from_numpy(case["corr"][:3]), seq0=2, min_n=2, since=1)))
    assert gpu.buffer.data_ptr() == first  # the buffers swap back
    other = sv.voxel_map_params(**repose.OTHER)  # a new box, size and capacity
    _agree(gpu, cpu, (gpu.repose(case["corr"], params=other), cpu.repose(case["corr"], params=other)))
    assert gpu.params == other and gpu._spare is None and gpu.buffer.numel() * 8 == eng.voxel_map_lib().sv_voxel_map_bytes(other["capacity"])
    with pytest.raises(TypeError):
        gpu.repose(case["corr"], min_weight=3)
    with pytest.raises(ValueError):
        gpu.repose(case["corr"][0])
    # merge under a pose: another session's map, whose world is turned and moved against this one's
    there = _rig_pair(BOX, [repose.cloud(BOX, 3, 250, 9)])
    pose = repose.rigid(np.random.default_rng(3), 0.4, 1.5)
    _agree(gpu, cpu, (gpu.merge(there[0], pose=pose, min_n=2), cpu.merge(there[1], pose=pose, min_n=2)))
    assert gpu.seq == 8 and _same_rows(_host(there[0].rows()), _host(there[1].rows()))
    for bad in (pose[:11], np.tile(pose, (2, 1))):
        with pytest.raises(ValueError):
            gpu.merge(there[0], pose=bad)
    # a carved map: the tombstones stay behind
    case = all_cases["tombstones_min_n_0"]
    gpu, cpu = _rig_pair(cases.BOX16, case["src"][1])
    xyz, n, counts, poses = case["carve"]["frames"]
    kw = dict(origin=(0.5, 8.5, 8.5), seq0=1, reach_m=16.0, margin=1, min_miss=1, ratio=0)
    gpu.carve(_cuda(xyz), _cuda(n), _cuda(counts), poses, **kw), cpu.carve(xyz, n, counts, poses, **kw)
    got, want = gpu.repose(case["corr"], min_n=0, min_rows=0), cpu.repose(case["corr"], min_n=0, min_rows=0)
    _agree(gpu, cpu, (got, want))
    assert [want[k] for k in STATS] == [7, 10, 0, 7] and gpu.stats()["claimed"] == 7


def _place_indices(sv, devices):
    """An index of five keyframes per device, re-posed under three corrections from sequence number 5 on; -> (indices, the poses wanted)."""
    import torch
    rigmod = util.pkg("rig")
    params = sv.place_params(20.0, rings=8, sectors=16)
    rng = np.random.default_rng(12)
    xyz = (rng.uniform(-15, 15, (5, 200, 3)) * [1, 1, 0.1]).astype(np.float32)
    counts = np.full(5, 200, np.int32)
    poses, corr = np.array([repose.rigid(rng, 0.5, 20.0) for _ in range(5)]), np.array([repose.rigid(rng, 0.1, 2.0) for _ in range(3)])
    seq = np.array([4, 5, 6, 7, 30])
    out = []
    for d in devices:
        ix = rigmod.PlaceIndex(params, 2, device=d)
        ix.add(ix.descriptor(torch.from_numpy(xyz).to(d), None, torch.from_numpy(counts).to(d)), seq, poses)
        ix.repose(corr, seq0=5)
        out.append(ix)
    want = sv.pose_repose(poses, seq, corr, 5)
    assert want[0].tobytes() == sv._pose_mul(corr[0], poses[0]).tobytes() and want[4].tobytes() == sv._pose_mul(corr[2], poses[4]).tobytes()
    return out, want


def _place_checks(sv, ix, want):
    assert ix.poses[:5].cpu().numpy().tobytes() == want.tobytes() and ix._pose_host.tobytes() == want.tobytes() and ix.count == 5
    best = np.array([[0, 0, 0, 1], [4, 3, 0, 1], [-1, 0, 0, 0]], np.int32)
    ok, guess = ix.guess({"best": ix._on_device(best, ix.words.dtype)})
    assert ok.tolist() == [True, True, False] and guess[:2].tobytes() == sv.place_guess(want[[0, 4]], best[:2, 1], 16).tobytes()


def test_the_place_index_on_cpu_tensors(sv):
    (ix,), want = _place_indices(sv, ["cpu"])
    _place_checks(sv, ix, want)


@pytest.mark.gpu
def test_the_place_index_on_both_devices(sv, eng):
    index, want = _place_indices(sv, ["cuda", "cpu"])
    for ix in index:
        _place_checks(sv, ix, want)


def _spec(eng, sv, params):
    return eng.voxel_map_spec(sv.voxel_map_params(**params))


@pytest.mark.gpu
def test_the_c_entry_refuses(sv, eng, all_cases):
    import torch
    L = eng.voxel_repose_lib()
    case = all_cases["table_smallest"]
    (dbuf, dwords), (sbuf, swords) = _engine_map(eng, sv, *case["dst"]), _engine_map(eng, sv, *case["src"])
    corr = _cuda(np.concatenate([case["corr"], np.zeros((1, 12))]))  # a spare row: an odd pointer into it stays inside the tensor
    stats = torch.full((6,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    keep = [t.clone() for t in (dbuf, sbuf, stats)]
    good = dict(dst=dbuf.data_ptr(), dst_bytes=dbuf.numel() * 8, dst_spec=_spec(eng, sv, case["dst"][0]), src=sbuf.data_ptr(), src_bytes=sbuf.numel() * 8,
                src_spec=_spec(eng, sv, case["src"][0]), corr=corr.data_ptr(), n_corr=2, seq0=0, stats=stats.data_ptr())

    def call(**change):
        a = dict(good, **change)
        spec = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731
        return L.sv_voxel_repose_device(a["dst"], a["dst_bytes"], spec(a["dst_spec"]), a["src"], a["src_bytes"], spec(a["src_spec"]), a["corr"], a["n_corr"], a["seq0"],
                                        1, 1, 0, a["stats"], torch.cuda.current_stream().cuda_stream)

    def spec_with(**words):
        s = _spec(eng, sv, BOX)
        for k, v in words.items():
            setattr(s, k, v)
        return s

    bad = []
    for which in ("dst", "src"):
        bad += [{which + "_spec": None}, {which: None}, {which: good[which] + 8}, {which + "_bytes": good[which + "_bytes"] - 8}, {which + "_bytes": 0}]
        bad += [{which + "_spec": spec_with(**w)} for w in (dict(size=0.0), dict(size=float("nan")), dict(capacity=0), dict(capacity=2 ** 26 + 1))]
    bad += [{"corr": None}, {"corr": good["corr"] + 4}, {"corr": good["dst"] + 64}, {"n_corr": 0}, {"n_corr": -1}, {"n_corr": 2 ** 22 + 1}, {"seq0": -1}, {"seq0": 2 ** 31 - 1}]
    bad += [{"src": good["dst"]}, {"src": good["dst"] + good["dst_bytes"] - 8, "src_bytes": 8 + good["src_bytes"]}]
    bad += [{"stats": good["stats"] + 4}, {"stats": good["dst"] + 64}, {"stats": good["src"] + good["src_bytes"] - 8}, {"stats": good["corr"] + 8}]
    for change in bad:
        eng.lib().sv_last_error(None)
        assert call(**change) == SV_ERR_ARG, change
        text = eng.lib().sv_last_error(None)
        assert text and b"sv_voxel_repose" in text, change
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((dbuf, sbuf, stats), keep))
    # and the same call, unchanged, is taken: with stats, and with none
    dst, src = _pair(sv, case)
    want = sv.voxel_map_repose(dst, src, case["corr"])
    assert call() == 0
    assert stats.cpu().tolist() == [want[k] for k in STATS] + [7, 7]
    table, head = _table(eng, sv, dbuf, dwords)
    assert all(np.array_equal(table[f], dst[f]) for f in WORDS) and head == (len(dst["key"]), dst["dropped"], False)
    sv.voxel_map_repose(dst, src, case["corr"], seq0=1)
    assert call(stats=None, seq0=1) == 0
    table, head = _table(eng, sv, dbuf, dwords)
    assert all(np.array_equal(table[f], dst[f]) for f in WORDS) and stats.cpu().tolist()[4:] == [7, 7]
    # the wrapper's own checks
    for kw in (dict(corr=case["corr"][0]), dict(corr=np.zeros((0, 12))), dict(corr=corr.float()), dict(corr=corr.cpu()), dict(seq0=-1), dict(seq0=2 ** 31 - 1), dict(seq0=0.5),
               dict(min_n=0.5), dict(since=2 ** 31)):
        with pytest.raises(ValueError):
            eng.voxel_map_repose(dbuf, dwords, sbuf, swords, **dict(dict(corr=case["corr"]), **kw))
    with pytest.raises(ValueError):
        eng.voxel_map_repose(dbuf, dwords, dbuf, dwords, case["corr"])


def _read_ply(path):
    with open(path, "rb") as f:
        data = f.read()
    at = data.index(b"end_header\n") + len(b"end_header\n")
    return data[:at].decode().splitlines(), data[at:]


def test_cli_argument_errors(sv, tmp_path):
    poses, ply, out = str(tmp_path / "poses.txt"), str(tmp_path / "ply"), str(tmp_path / "drive.ply")
    with open(poses, "w") as f:
        f.write("0 0 0\n")
    for bad in (["--voxel-repose", poses], ["--batch", "2", "--ply", ply, "--voxel", "0.2", "--voxel-repose", poses]):
        with pytest.raises(SystemExit):
            sv.main(["-k", str(tmp_path / "kitti")] + bad)
    assert not os.path.exists(out) and not os.path.exists(ply)


@pytest.mark.gpu
def test_cli_repose(sv, eng, tmp_path, capsys):
    """--voxel-repose at the end of a run against the same drive through the CPU object."""
    from PIL import Image
    from test_occupancy_map import H, W, _drive_frames
    n = 4
    ls, rs = _drive_frames(n)
    xyyaw = np.array([[0.0, 0.0, 0.0], [0.8, 0.05, 0.03], [1.6, 0.1, 0.06], [2.4, 0.1, 0.09]])
    fixed = xyyaw + np.array([[0.0, 0.0, 0.0], [0.1, -0.1, 0.01], [0.2, -0.2, 0.02], [0.3, -0.3, 0.03]])
    rigmod = util.pkg("rig")
    rig = rigmod.StereoRig(W, H)
    try:
        cloud = rig.voxel_clouds(_cuda(ls[..., ::-1].copy()), _cuda(rs[..., ::-1].copy()), 0.2, sv.CLI_CLOUD_CROP[0], sv.CLI_CLOUD_CROP[1],
                                 transform=(sv.CAMERA_TO_VEHICLE, None), capacity=65536)
    finally:
        rig.close()
    xyz, color, cnt, counts = (t.cpu().numpy() for t in cloud)
    lo, hi = sv.cli_voxel_map_box(xyyaw)
    world = rigmod.VoxelMap(lo, hi, 0.2, sv.CLI_VOXEL_MAP_CAPACITY, device="cpu")
    went = sv.voxel_map_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2])
    for i in (0, 2):
        world.update(xyz[i:i + 2], color[i:i + 2], cnt[i:i + 2], counts[i:i + 2], went[i:i + 2])
    lo2, hi2 = sv.cli_voxel_map_box(fixed)
    stats = world.repose(sv.pose_corrections(went, sv.voxel_map_pose(fixed[:, 0], fixed[:, 1], fixed[:, 2])),
                         params=sv.voxel_map_params(lo2, hi2, 0.2, sv.CLI_VOXEL_MAP_CAPACITY))
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    for name, rows in (("poses.txt", xyyaw), ("fixed.txt", fixed)):
        with open(tmp_path / name, "w") as f:
            f.write("".join("%r %r %r\n" % tuple(float(v) for v in row) for row in rows))
    out = str(tmp_path / "drive.ply")
    capsys.readouterr()
    sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt"), "--voxel-map", out,
             "--voxel-repose", str(tmp_path / "fixed.txt")])
    said = [line for line in capsys.readouterr().out.splitlines() if line.startswith("voxel map re-posed")]
    want = _host(world.rows())
    assert said == ["voxel map re-posed: %s; %d voxels written to %s" % (sv.cli_voxel_carry_text(stats), want["count"], str(tmp_path / "drive.reposed.ply"))]
    assert stats["carried"] > 1000
    head, payload = _read_ply(str(tmp_path / "drive.reposed.ply"))
    rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert head[2] == "element vertex %d" % want["count"]
    assert np.array_equal(rec["xyz"].view(np.uint32), want["xyz"].view(np.uint32)) and np.array_equal(rec["rgb"], want["color"][:, 2::-1])
