"""The GPU lattice filters - k_filter_classify, k_filter_resolve, k_filter_vertical, k_filter_horizontal, k_filter_collect and
k_filter_corners of csrc/kernels.hip - on the lattices of tests/lattice_cases.py, which are painted point by point: chains of uncertain
points that three refinement rounds cannot finish, uncertain points on both sides of a classify block's end, windows that hang over
every edge, lines of every length at which the redundancy walk and its strips turn over, lists of 0 .. 3 points, tied and far corner
searches, a lattice that keeps every point.  The lists are compared with the oracle's (orc_support_filter) byte for byte.

CPU: the constants the cases restate are the source's; the cases' own numpy restatement of the filters equals the oracle on every case,
and shows what each case is aimed at; the host filters on the chains, the full lattice and the ties; the refusals of
sv_gpu_support_filter (they come before the first HIP call).
GPU: every case alone through sv_gpu_support_filter with the resolve step's statistics; every case in launches of 2 and 5 lattices, first,
in the middle and last, behind another launch in the same workspace; four lattices through sv_debug_inject's "lattice" stage into
keep_debug handles with the filters on the GPU and on the host; the refusals of that stage."""
import ctypes
import os
import re

import numpy as np
import pytest

import lattice_cases as lc
import util
from pyoracle import ElasParams

KERNELS = os.path.join(util.ROOT, util.PKG, "csrc", "kernels.hip")
_WANT = {}


def _oracle_list(oracle, over, lattice, W, H):
    """orc_support_filter's list for a lattice, computed once and left unchanged."""
    key = (tuple(sorted(over.items())), W, H, lattice.shape, lattice.tobytes())
    if key not in _WANT:
        L = oracle.lib
        L.orc_support_filter.argtypes = [ctypes.POINTER(ElasParams), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
        L.orc_support_filter.restype = ctypes.c_int
        po = lc.params(ElasParams, over)
        a = np.array(lattice, np.int16)
        out = np.zeros((a.size + 6, 3), np.int32)
        n = L.orc_support_filter(ctypes.byref(po), a.ctypes.data, W, H, out.ctypes.data, out.shape[0])
        assert n >= 0
        want = out[:n].copy()
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def _want(oracle, case):
    return _oracle_list(oracle, case.over, case.lattice, case.W, case.H)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def host_eng():
    util.pkg("build").build()
    return util.pkg("engine")


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_sources():
    src = open(KERNELS).read()
    assert re.search(r"#define FCL_THREADS (\d+)", src).group(1) == re.search(r"#define FLT_THREADS (\d+)", src).group(1) == str(lc.BLOCK)
    strip = src[src.index("static int filter_strip("):]
    assert re.search(r"int s = (\d+);", strip).group(1) == str(lc.STRIP)
    walk = src[src.index("void redundancy_walk("):]
    assert re.search(r"p0 \+= (\d+)\)", walk).group(1) == str(lc.WALK)
    assert re.search(r"round < (\d+) && left", src).group(1) == str(lc.ROUNDS)
    assert "dist < %d" % lc.FAR in src
    assert lc.LINKS > 200 and lc.LINKS - 3 > 4 * lc.ROUNDS  # (a round settles one link per wavefront of the resolve workgroup at the most)


def test_the_cases_keep_the_contract():
    assert sorted(lc.FAMILIES) == sorted(["full", "chains", "blocks", "edges", "walks", "collect", "random"])
    assert len(lc.FAMILIES["random"]) == 24
    for c in lc.CASES.values():
        d = c.lattice
        assert d.dtype == np.int16 and d.min() >= -1 and d.max() <= lc.DISP_MAX and not d[0].any() and not d[:, 0].any(), c.name
        assert d.size <= 70000 and c.aim, c.name
        win, thr, need, _ = c.filter_params
        assert 0 <= win <= 5 and 0 <= need <= 60 and 0 <= thr < 4096, c.name
    sides = [s for n in lc.FAMILIES["random"] for s in lc.CASES[n].lattice.shape]
    assert min(sides) >= 8 and max(sides) <= 140
    assert {lc.CASES[n].Hc for n in lc.FAMILIES["blocks"]} >= {2, 3, 11, 16, 17, 64, 65, 255, 256, 257}
    for lines in ({lc.CASES[n].Hc for n in lc.FAMILIES["walks"] if "_v" in n}, {lc.CASES[n].Wc for n in lc.FAMILIES["walks"] if "_h" in n}):
        assert lines >= set(lc.LINES)
    for strips in ({lc.CASES[n].Wc for n in lc.FAMILIES["walks"] if "_v" in n}, {lc.CASES[n].Hc for n in lc.FAMILIES["walks"] if "_h" in n}):
        assert strips >= set(lc.STRIPS)
    seen = {(c.filter_params[0], c.filter_params[2], c.filter_params[1]) for c in (lc.CASES[n] for n in lc.FAMILIES["edges"])}
    assert seen == {(w, n, t) for w in (0, 1, 5) for n in (0, 1, 60) for t in (0, 4095)}


@pytest.mark.parametrize("family", sorted(lc.FAMILIES))
def test_the_restatement_is_the_oracle(oracle, family):
    """lattice_cases.model - classification, the points it leaves open in scan order, the two redundancy passes, collection, corners - gives
    the oracle's list on every case: what it says about a case below is said about the reference."""
    for name in lc.FAMILIES[family]:
        c = lc.CASES[name]
        got, want = lc.model(c), _want(oracle, c)
        assert _same(got, want), (name, got.shape, want.shape)


def _unc_blocks(state, Hc):
    idx = np.flatnonzero(state.T.ravel() == lc.UNC)  # scan-order indices u * Hc + v
    return np.bincount(idx // lc.BLOCK, minlength=(state.size + lc.BLOCK - 1) // lc.BLOCK)


def _check_aim(c):
    win, thr, need, corners = c.filter_params
    x = c.expect
    _, _, state = lc.classify(c.lattice, win, thr, need)
    pts, A, B, C, ties = lc.model(c, parts=True)
    if "count" in x:
        assert len(pts) == x["count"], len(pts)
    if "n_main" in x:
        assert len(pts) - 6 * corners == x["n_main"], len(pts)
    if c.family == "full":
        max_pts = (c.Wc - 1) * (c.Hc - 1) + 6
        assert len(pts) == max_pts and len(pts) > max(4096, c.Wc * c.Hc // 6)  # the last word of the blob, and the separate copy of a long list
    if "cells" in x:
        cells = x["cells"]
        st = [state[v, u] for u, v in cells]
        assert st.count(lc.UNC) == x["unc"] and len(cells) == lc.LINKS, st.count(lc.UNC)
        assert sum(A[v, u] >= 0 for u, v in cells) == x["kept"]
        # a chain: every uncertain cell has exactly one consistent earlier neighbour that is not kept for sure - its predecessor in
        # the chain - and its fate is that neighbour's, so no round can settle it before the predecessor is settled
        unc = [(u, v) for u, v in cells if state[v, u] == lc.UNC]
        first = unc[0]
        for u, v in unc[1:]:
            early = [(u2, v2) for u2 in range(max(u - win, 0), u + 1) for v2 in range(max(v - win, 0), min(v + win, c.Hc - 1) + 1)
                     if (u2 < u or v2 < v) and c.lattice[v2, u2] >= 0 and abs(int(c.lattice[v2, u2]) - int(c.lattice[v, u])) <= thr]
            open_ = [q for q in early if state[q[1], q[0]] == lc.UNC]
            assert len(open_) == 1 and open_[0] in cells, (u, v, early)
            assert (A[v, u] >= 0) == (A[open_[0][1], open_[0][0]] >= 0)
        assert first in cells
        if x.get("sparse_blocks"):
            per = _unc_blocks(state, c.Hc)
            mine = np.bincount([(u * c.Hc + v) // lc.BLOCK for u, v in unc], minlength=len(per))
            used = np.flatnonzero(mine)
            span = per[used[0]:used[-1] + 1]
            assert mine.max() == 1 and span.max() <= 3   # (the other ones are row 0's: the border's own chain)
            assert (span == 0).sum() >= 20, "classify blocks without uncertain points between blocks that have some"
        elif len({u for u, v in cells}) == 1:   # down a column: consecutive indices
            assert len({(u * c.Hc + v) // lc.BLOCK for u, v in unc}) <= 2
        if x.get("border"):
            bare = np.array(c.lattice)
            bare[:, 0] = -1   # (outside the contract: the restatement only)
            A0 = lc.drop_inconsistent(bare, win, thr, need)
            assert sum(A0[v, u] >= 0 for u, v in cells) == 0, "without the zero border the chain falls"
    if "unc_at" in x:
        flat = state.T.ravel()
        assert all(flat[i] == lc.UNC for i in x["unc_at"]), [int(flat[i]) for i in x["unc_at"]]
        assert len(_unc_blocks(state, c.Hc)) >= 3
    if "unc_blocks" in x:
        per = _unc_blocks(state, c.Hc)
        assert list(np.flatnonzero(per)) == x["unc_blocks"] and x["unc_blocks"][-1] == len(per) - 1 and len(per) >= 3, per
    if "keeps_all" in x:
        assert x["keeps_all"] == bool((A == c.lattice).all())
        assert (c.lattice[1, 1:] >= 0).all() and (c.lattice[1:, 1] >= 0).all() and (c.lattice[-1, 1:] >= 0).all() and (c.lattice[1:, -1] >= 0).all()
        if need == 60 and win < 5:
            assert (A < 0).all()   # (a window of at most nine points)
        if need == 60 and win == 5 and thr == 4095:
            assert (A >= 0).any() and (A < 0).any() and (A[c.lattice >= 0] < 0).any()
    if c.family == "walks" and "through" not in x:
        assert (A == c.lattice).all(), "nothing is needed: the redundancy passes see the painted lattice"
    if "triples" in x:
        D_in, D_out = (A, B) if x["vertical"] else (B, C)
        for (u, v), (a, b) in x["triples"]:
            along = (lambda k: (v + k, u)) if x["vertical"] else (lambda k: (v, u + k))
            head, mid, tail = along(0), along(a), along(a + b)
            assert D_in[head] == D_in[mid] == D_in[tail] >= 0
            assert D_out[head] >= 0 and D_out[tail] >= 0 and (D_out[mid] < 0) == (a <= 5 and b <= 5), ((u, v), (a, b))
        runs = {}
        line_of = (lambda D, k: D[:, k]) if x["vertical"] else (lambda D, k: D[k, :])
        for L in range(2, 13):
            before, after = line_of(D_in, L), line_of(D_out, L)
            assert (before == 20 + 3 * L).sum() == L
            runs[L] = int((after == 20 + 3 * L).sum())
        assert runs[2] == 2 and all(runs[L] < L for L in range(3, 13)), runs
        assert (line_of(D_out, 13)[3:20] >= 0).sum() < 17 and (line_of(D_out, 14)[3:20] >= 0).sum() < 17  # apart by 1: matches; by 2: the equal ones two further
    if "through" in x:
        (pu, pv), (xu, xv) = x["through"]["P"], x["through"]["X"]
        assert c.lattice[xv, xu] >= 0 and A[xv, xu] < 0 and state[xv, xu] == lc.DROP and C[pv, pu] >= 0
        kept_all = lc.drop_redundant_vertical(np.array(c.lattice, np.int32))
        assert kept_all[pv, pu] < 0, "with X in place P has a match on both sides"
    if "collect_blocks" in x:
        idx = [u * c.Hc + v for u, v in np.argwhere(C.T[1:, 1:] >= 0) + 1]
        assert sorted({i // lc.BLOCK for i in idx}) == x["collect_blocks"] and (c.Wc * c.Hc + lc.BLOCK - 1) // lc.BLOCK == 10
    if c.name.startswith("collect_") and x.get("n_main", 0) >= 1 and c.name[8].isdigit():
        assert lc.DISP_MAX in pts[:x["n_main"], 2]
    if "tied_corners" in x:
        for i in x["tied_corners"]:
            best, tied = ties[i]
            assert len(tied) == 2 and pts[tied[0], 2] > pts[tied[1], 2] and pts[x["n_main"] + i, 2] == pts[tied[0], 2], (i, best, tied)
    if "far_corners" in x:
        for i in range(4):
            best, tied = ties[i]
            assert (best >= lc.FAR and not tied and pts[x["n_main"] + i, 2] == 0) if i in x["far_corners"] else (best < lc.FAR and pts[x["n_main"] + i, 2] > 0), (i, best)
        assert min((c.W - 1 - int(p[0])) ** 2 for p in pts[:x["n_main"]]) > lc.FAR


@pytest.mark.parametrize("family", sorted(lc.FAMILIES))
def test_the_cases_realise_what_they_are_aimed_at(family):
    """Every expectation of every case of the family, on the cases' restatement of the classification and of the filters."""
    for name in lc.FAMILIES[family]:
        try:
            _check_aim(lc.CASES[name])
        except AssertionError as err:
            raise AssertionError("%s: %s" % (name, err))


def test_random_lattices_leave_work_for_every_step():
    """The random family has uncertain points in most lattices, some in many classify blocks, and lists with and without corners."""
    n_unc, corners = [], set()
    for name in lc.FAMILIES["random"]:
        c = lc.CASES[name]
        win, thr, need, cor = c.filter_params
        n_unc.append(int((lc.classify(c.lattice, win, thr, need)[2] == lc.UNC).sum()))
        corners.add(cor)
    assert sum(n > 0 for n in n_unc) >= 16 and max(n_unc) > 500 and corners == {0, 1}, n_unc


_HOST_CASES = ["full_80x60", "corner_ties", "corner_far"] + lc.FAMILIES["chains"]


@pytest.mark.parametrize("name", _HOST_CASES)
def test_host_filters_on_chains_full_lattice_and_ties(host_eng, oracle, name):
    """The host filters - plain and shared between 2 and 5 threads - have not seen these lattices either."""
    c = lc.CASES[name]
    pe, want = lc.params(host_eng.SvParams, c.over), _want(oracle, c)
    for threads in (0, 2, 5):
        got = host_eng.host_support_filter(pe, np.array(c.lattice), c.W, c.H, threads=threads)
        assert _same(got, want), (name, threads, got.shape, want.shape)


def _entry(eng):
    L = eng.lib()
    L.sv_gpu_support_filter.argtypes = [ctypes.POINTER(eng.SvParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p]
    L.sv_gpu_support_filter.restype = ctypes.c_int
    return L


def test_entry_refusals(host_eng):
    """One assertion per rule of sv_gpu_support_filter: SV_ERR_ARG, a text, and the outputs untouched (the rules come before the first HIP call)."""
    eng = host_eng
    L = _entry(eng)
    good = lc.blank(20, 16)
    good[5, 7] = 30

    def call(over=None, lattice=good, W=100, H=80, cap=None):
        p = lc.params(eng.SvParams, dict(over or {}, candidate_stepsize=5))
        lat = np.ascontiguousarray(lattice, np.int16)
        cap = (lat.shape[-1] - 1) * (lat.shape[-2] - 1) + 6 if cap is None else cap
        out, counts = np.full((max(cap, 1), 3), -7, np.int32), np.full(1, -7, np.int32)
        rc = L.sv_gpu_support_filter(ctypes.byref(p), lat.ctypes.data, None, 1, W, H, out.ctypes.data, cap, counts.ctypes.data, None)
        assert (out == -7).all() and counts[0] == -7
        return rc, L.sv_last_error(None).decode()

    def refused(what, **kw):
        rc, text = call(**kw)
        assert rc == -1 and text.startswith("sv_gpu_support_filter") and what in text, (rc, text)

    refused("incon_window_size", over=dict(incon_window_size=6))
    refused("incon_min_support", over=dict(incon_min_support=61))
    refused("incon_threshold", over=dict(incon_threshold=4096))
    refused("cap", cap=19 * 15 + 5)
    for bad in (-2, lc.DISP_MAX + 1):
        lat = good.copy()
        lat[15, 19] = bad
        refused("neither -1 nor a disparity", lattice=lat)
    for where in ((0, 3), (3, 0), (0, 0)):
        for bad in (-1, 1):
            lat = good.copy()
            lat[where] = bad
            refused("row 0 / column 0", lattice=lat)


def test_entry_refuses_a_lattice_beyond_the_block_table(host_eng):
    eng = host_eng
    L = _entry(eng)
    src = open(KERNELS).read()
    limit = int(re.search(r"#define RSV_MAX_BLOCKS (\d+)", src).group(1)) * lc.BLOCK
    Wc, Hc = 8190, 257
    assert Wc * Hc > limit
    p = lc.params(eng.SvParams, dict(candidate_stepsize=1))
    lat = lc.blank(Wc, Hc)
    cap = (Wc - 1) * (Hc - 1) + 6
    counts = np.full(1, -7, np.int32)
    out = np.zeros((1, 3), np.int32)   # (never written: the call is refused before it looks at cap's worth of memory)
    rc = L.sv_gpu_support_filter(ctypes.byref(p), lat.ctypes.data, None, 1, Wc, Hc, out.ctypes.data, cap, counts.ctypes.data, None)
    assert rc == -1 and "block table" in L.sv_last_error(None).decode() and counts[0] == -7


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    util.pkg("build").build()
    return util.pkg("engine")


_STATS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(lc.CASES))
def test_case_alone(eng, oracle, name):
    """A launch of one lattice: the oracle's list and count; as many uncertain points as the classification leaves; a sequential rest for
    the chains and none where nothing is uncertain."""
    c = lc.CASES[name]
    want = _want(oracle, c)
    lists, counts, stats = eng.gpu_support_filter(lc.params(eng.SvParams, c.over), c.lattice, c.W, c.H, stats=True)
    print("%s: count %d, stats (n_unc, rounds, n_rest) %s" % (name, counts[0], stats[0].tolist()))
    _STATS[name] = stats[0].tolist()
    assert counts[0] == len(want) and _same(lists[0], want), (name, int(counts[0]), len(want))
    win, thr, need, _ = c.filter_params
    n_unc = int((lc.classify(c.lattice, win, thr, need)[2] == lc.UNC).sum())
    assert stats[0, 0] == n_unc, (name, stats[0].tolist(), n_unc)
    assert 0 <= stats[0, 1] <= lc.ROUNDS and 0 <= stats[0, 2] <= n_unc
    if n_unc == 0:
        assert stats[0, 1] == 0 and stats[0, 2] == 0
    if stats[0, 1] < lc.ROUNDS:
        assert stats[0, 2] == 0
    if c.expect.get("chain"):
        assert stats[0, 2] > 0, (name, stats[0].tolist())


_GROUPS = {}
for _c in lc.CASES.values():
    _GROUPS.setdefault(_c.key(), []).append(_c.name)
_GROUP_KEYS = sorted(_GROUPS, key=repr)


@pytest.mark.gpu
@pytest.mark.parametrize("g", range(len(_GROUP_KEYS)), ids=lambda g: _GROUPS[_GROUP_KEYS[g]][0])
def test_batches_and_a_used_workspace(eng, oracle, g):
    """Launches of 2 and 5 lattices of one size: every case of the size at pair 0, in the middle and last, the other pairs other cases of
    that size, a dense lattice, an empty one and the case turned round.  Each launch runs behind another in the same workspace and output
    buffers - the same lattices, or dense ones in front of a batch that has sparse ones - and every pair must still give the oracle's
    list, with the statistics of its own launch of one."""
    names = _GROUPS[_GROUP_KEYS[g]]
    first = lc.CASES[names[0]]
    pe = lc.params(eng.SvParams, first.over)
    win, thr, need, _ = first.filter_params
    pool = [lc.CASES[n].lattice for n in names] + [lc.dense_filler(first), lc.sparse_filler(first), lc.turned_filler(first)]
    dense = lc.dense_filler(first)
    turn = 0
    for ci, name in enumerate(names):
        c = lc.CASES[name]
        others = [m for i, m in enumerate(pool) if i != ci]
        for n in (2, 5):
            for pos in sorted({0, n // 2, n - 1}):
                batch = [others[(turn + k) % len(others)] for k in range(n)]
                batch[pos] = c.lattice
                turn += 1
                batch = np.stack(batch)
                prime = batch if turn % 2 else np.stack([dense] * n)
                lists, counts, stats = eng.gpu_support_filter(pe, batch, c.W, c.H, stats=True, prime=prime)
                for i in range(n):
                    want = _oracle_list(oracle, c.over, batch[i], c.W, c.H)
                    assert counts[i] == len(want) and _same(lists[i], want), (name, n, pos, i, int(counts[i]), len(want))
                    assert stats[i, 0] == int((lc.classify(batch[i], win, thr, need)[2] == lc.UNC).sum()), (name, n, pos, i)
                if c.expect.get("chain"):
                    assert stats[pos, 2] > 0, (name, n, pos, stats.tolist())


_ENGINE_CASES = ["full_80x60", "chain_col_keep", "collect_2_c0", "collect_3_c0"]


def _stage(e, name):
    try:
        return e.debug(name)
    except KeyError:
        return None


@pytest.mark.gpu
@pytest.mark.parametrize("shape_of", ["full_80x60", "chain_col_keep", "collect_2_c0"])
def test_injected_lattices_through_the_engine(eng, oracle, shape_of):
    """Two keep_debug handles per image size, lattice filters on the GPU and on the host: the painted lattice is what dcan_raw reads back,
    the support list is the oracle's, the status is its length, and everything behind it is the same on both handles, byte for byte.  The
    full lattice's list is longer than the head that is copied with the counts; after the hook is cleared a pair is itself again."""
    names = [n for n in _ENGINE_CASES if lc.CASES[n].key()[:3] == lc.CASES[shape_of].key()[:3] and lc.CASES[n].over == lc.CASES[shape_of].over]
    if shape_of == "collect_2_c0":
        assert names == ["collect_2_c0", "collect_3_c0"]
    c0 = lc.CASES[shape_of]
    L, R = util.pkg("synth").make_pair(11, c0.H, c0.W, 24)
    handles = [eng.StereoEngine(c0.W, c0.H, lc.params(eng.SvParams, c0.over), keep_debug=True, gpu_filter=on, n_workers=2) for on in (True, False)]
    try:
        assert [e.query()["gpu_lattice_filter"] for e in handles] == [1, 0]
        for name in names:
            c = lc.CASES[name]
            want = _want(oracle, c)
            got = []
            for e in handles:
                e.debug_inject("lattice", np.array(c.lattice))
                d1, d2, status = e.process_host(L, R)
                assert _same(e.debug("dcan_raw"), c.lattice.ravel()), (name, "dcan_raw is not the painted lattice")
                assert e.debug("dcan_dims").tolist() == [c.Wc, c.Hc]
                assert _same(e.debug("support"), want.ravel()), (name, e.debug("support").size // 3, len(want))
                assert int(status[0]) == len(want), (name, status)
                got.append(dict({s: _stage(e, s) for s in util.STAGES}, d1=d1.copy(), d2=d2.copy()))
            for k in got[0]:
                a, b = got[0][k], got[1][k]
                assert (a is None) == (b is None) and (a is None or _same(a, b)), (name, k)
            if name == "full_80x60":
                max_pts = (c.Wc - 1) * (c.Hc - 1) + 6
                assert len(want) == max_pts > min(max_pts, max(4096, c.Wc * c.Hc // 6)), "the list must take the separate copy of a long list"
        po =lc.params(ElasParams, c0.over)
        n_own = oracle.run_stages(po, L, R)
        own = {k: oracle.stage(k).copy() for k in ("dcan_raw", "support")}
        own_final = oracle.stage("final1", (c0.H, c0.W)).copy() if n_own >= 3 else None
        for e in handles:
            e.debug_inject("lattice", None, None)
            d1, _, status = e.process_host(L, R)
            assert int(status[0]) == n_own and _same(e.debug("dcan_raw"), own["dcan_raw"]) and _same(e.debug("support"), own["support"])
            if own_final is not None:
                assert _same(d1[0], own_final)
    finally:
        for e in handles:
            e.close()


@pytest.mark.gpu
def test_lattice_stage_refusals(eng):
    """No keep_debug, another lattice size, values outside the contract, a non-zero border; the float-map entry does not take the stage."""
    W, H = 100, 80
    ok = lc.blank(20, 16)
    p = lc.params(eng.SvParams, dict(candidate_stepsize=5))
    e = eng.StereoEngine(W, H, p, n_workers=2)
    try:
        with pytest.raises(eng.StereoError, match="keep_debug"):
            e.debug_inject("lattice", ok)
    finally:
        e.close()
    e = eng.StereoEngine(W, H, p, keep_debug=True, n_workers=2)
    try:
        for bad in (lc.blank(21, 16), lc.blank(20, 15), lc.blank(16, 20)):
            with pytest.raises(eng.StereoError, match="lattice is 20 x 16"):
                e.debug_inject("lattice", bad)
        for bad in (ok.astype(np.float32), ok.astype(np.int32), ok.ravel(), ok.tolist()):
            with pytest.raises(ValueError):
                e.debug_inject("lattice", bad)
        with pytest.raises(ValueError):
            e.debug_inject("lattice", ok, ok)
        for val in (-2, lc.DISP_MAX + 1, 32767, -32768):
            m = ok.copy()
            m[15, 19] = val
            with pytest.raises(eng.StereoError, match="neither -1 nor a disparity"):
                e.debug_inject("lattice", m)
        for where in ((0, 5), (5, 0)):
            for val in (-1, 3):
                m = ok.copy()
                m[where] = val
                with pytest.raises(eng.StereoError, match="row 0 / column 0"):
                    e.debug_inject("lattice", m)
        f = np.full((H, W), -10, np.float32)
        with pytest.raises(eng.StereoError, match="sv_debug_inject_lattice"):
            e._check(eng.lib().sv_debug_inject(e._h, b"lattice", f.ctypes.data, f.ctypes.data))
        for fine in (-1, 0, lc.DISP_MAX):
            m = ok.copy()
            m[15, 19] = fine
            e.debug_inject("lattice", m)
        e.debug_inject("lattice", None, None)
    finally:
        e.close()
