"""GPU (MI355X): the device triangulation (csrc/delaunay_gpu.hip) and the whole pipeline on degenerate support sets - the structured
sets and pairs of tests/degenerate_sets.py.  The CPU emulations of the same kernels on the same sets (tests/test_sanitizers.py, with a
trip-count bound on every merge loop) come first; the point-set tests here come before the pipeline tests.  Tolerance 0."""
import numpy as np
import pytest

import degenerate_sets
import util
from pyoracle import ElasParams

pytestmark = pytest.mark.gpu

N_SETS = 592
LARGE_MAX = degenerate_sets.DG_SUB_MAX << 6  # delaunay_gpu.hip: vertices the cut path takes (DG_SUB_MAX << DG_CUT_MAX)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return util.pkg("engine")


@pytest.fixture(scope="module")
def corpus(eng):
    """[(name, xy, the host stage's triangle list)] - the host stage equals the oracle on every set (tests/test_degenerate_host.py)"""
    return [(name, xy, eng.host_delaunay(xy)) for name, xy in degenerate_sets.sets()]


def _gpu_sets(eng, corpus, reps):
    done = refused = 0
    for name, xy, want in corpus:
        if len(xy) > LARGE_MAX:  # the 4K lattice: more vertices than the kernels take - the launcher must say so, not launch
            with pytest.raises(eng.StereoError):
                eng.gpu_delaunay(xy, reps=reps)
            refused += 1
        else:
            got, _ = eng.gpu_delaunay(xy, reps=reps)
            assert got.shape == want.shape and np.array_equal(got, want), name
        done += 1
    return done, refused


@pytest.mark.parametrize("reps", [1, 3])
def test_gpu_delaunay_structured_sets(eng, corpus, reps):
    """k_delaunay (sets of up to 4000 points whole in LDS) and k_dgl_subtrees / k_dgl_top (larger ones) against the host stage; reps: the
    same set several times in one launch."""
    assert _gpu_sets(eng, corpus, reps) == (N_SETS, 2)


# sub_max -> (sets the launcher must refuse, {cut depth: sets}) - counted from the corpus by the kernels' documented rule: a set of n > sub_max
# points with m distinct ones is cut at the smallest depth c with ceil(m / 2^c) <= sub_max and refused when c > 6 (depth 0: a set whose
# coincident points bring it below the limit after all).  tests/test_degenerate_host.py::test_cut_path_expectations recounts them.
CUT_EXPECT = {6: (76, {0: 20, 1: 64, 2: 46, 3: 20, 4: 90, 5: 28, 6: 80}),
              50: (44, {1: 110, 2: 12, 3: 80, 4: 12, 5: 12, 6: 4}),
              333: (2, {1: 12, 2: 12, 3: 4, 4: 42, 6: 4})}


@pytest.mark.parametrize("sub_max", sorted(CUT_EXPECT))
def test_gpu_delaunay_cut_path_structured_sets(eng, corpus, monkeypatch, sub_max):
    """The cut path with the subtree limit lowered: every set of more than sub_max points is built as 2^c subtrees in LDS plus the
    merges above the cut in global memory - wholly collinear subtrees and upper merges included.  With 50 (and with 6) the corpus reaches
    every depth from 1 to 6.  Sets that would need more than 2^6 subtrees are refused by the launcher (DG_CUT_MAX): a refusal is an
    error from gpu_delaunay, anything else must be the host's list."""
    monkeypatch.setenv("SV_DG_SUBMAX", str(sub_max))
    done, refused, depths = 0, 0, {}
    for name, xy, want in corpus:
        try:
            got, _ = eng.gpu_delaunay(xy, reps=2)
        except eng.StereoError:
            refused += 1
        else:
            assert got.shape == want.shape and np.array_equal(got, want), name
            if len(xy) > sub_max:
                c = degenerate_sets.cut_depth(len(np.unique(xy, axis=0)), sub_max)
                depths[c] = depths.get(c, 0) + 1
        done += 1
    assert done == N_SETS and (refused, depths) == CUT_EXPECT[sub_max]
    if sub_max == degenerate_sets.CUT_SUB_MAX:
        assert set(depths) == {1, 2, 3, 4, 5, 6}


def test_gpu_kd_order_structured_sets(eng, corpus):
    """dg_prepare against the host's preparation on every set that is a vertex set of a 1242 x 375 image's support lattice with
    disparities up to 1023 (rows at multiples of 5, x from -1023) and within DG_PREP_MAX.  Coincident vertices (the header's rule): with
    equal disparities they are one support point twice - the lowest id survives, up to 16 of them; without disparities, with different
    ones, or with more than 16, the set is handed back (None)."""
    W, H, step, D = 1242, 375, 5, 1023
    done = merged = handed_back = 0
    for name, xy, _ in corpus:
        if len(xy) > degenerate_sets.DG_PREP_MAX or (xy[:, 1] % step).any() or xy[:, 1].max() >= H or xy[:, 0].max() >= W + D or xy[:, 0].min() < -D:
            continue
        want = eng.host_kd_order(xy)
        dup = len(xy) - len(want)
        got = eng.gpu_kd_order(xy, W, H, step, D, disp=np.zeros(len(xy), np.int32))
        if dup == 0:
            assert got is not None and np.array_equal(got, want), name
            assert np.array_equal(eng.gpu_kd_order(xy, W, H, step, D), want), name
        elif dup > 16:
            assert got is None, name
        else:
            keys = xy[:, 0].astype(np.int64) * 100000 + xy[:, 1]
            assert got is not None and np.array_equal(xy[got], xy[want]), name
            assert all(g == np.flatnonzero(keys == keys[g])[0] for g in got), name
            assert eng.gpu_kd_order(xy, W, H, step, D) is None, name  # no disparities: not known to be interchangeable
            twin = int(np.flatnonzero(np.bincount(np.unique(keys, return_inverse=True)[1])[np.unique(keys, return_inverse=True)[1]] > 1)[0])
            dd = np.zeros(len(xy), np.int32)
            dd[twin] = 1
            assert eng.gpu_kd_order(xy, W, H, step, D, disp=dd) is None, name  # one twin with another disparity
            merged += 1
        done += 1
    by_name = {name: xy for name, xy, _ in corpus}
    for name in ("collinear_row_300", "lattice_8x8", "strip_2_rows_50_negx_shuffled"):  # 17 coincident vertices: one more than the kernel merges
        xy = np.ascontiguousarray(np.concatenate([by_name[name], by_name[name][:17]]))
        assert eng.gpu_kd_order(xy, W, H, step, D, disp=np.zeros(len(xy), np.int32)) is None, name
        xy = np.ascontiguousarray(xy[:-1])  # 16: merged
        got, want = eng.gpu_kd_order(xy, W, H, step, D, disp=np.zeros(len(xy), np.int32)), eng.host_kd_order(xy)
        assert got is not None and np.array_equal(xy[got], xy[want]), name
        handed_back += 1
    assert (done, merged, handed_back) == (370, 32, 3)


# ---- whole pairs whose support set is degenerate ------------------------------------------------------------------------------------
# Which handle can triangulate where is the engine's rule (engine.cpp, sv_create): the device triangulation and the resident path exist
# only on handles with chunk >= 4 and without keep_debug.  So the stage-by-stage comparison (keep_debug) and the chunk-1 latency handles
# run the host triangulation whatever is asked for - asserted below, not parametrised - and host / GPU / resident on and off are
# crossed with the batch handles, where every case asserts from sv_query which path the handle took.

PAIRS = [c[0] for c in degenerate_sets.pair_cases()]
STAGES = util.STAGES
# pairs that share image size and parameters share a handle (and a batch)
GROUPS = [["band_row_320x120", "band_col_320x120"], ["band_row_203x97"], ["band_row_sub_320x120"], ["band_col_161x140"], ["full_lattice_170x90"], ["strip_two_rows_240x32"]]
BATCH_MODES = {"host": ("host", None, 0, 0), "gpu_resident": ("gpu", None, 1, 1), "gpu_not_resident": ("gpu", False, 1, 0)}  # triangulation, resident, queried gpu_triangulation, resident


@pytest.fixture(scope="module")
def wanted(oracle):
    """name -> (L, R, n_support, {stage: array}, D1, D2) of the oracle"""
    out = {}
    for name in PAIRS:
        L, R, _, _ = degenerate_sets.make_pair(name)
        p = degenerate_sets.pair_params(ElasParams, name)
        n = oracle.run_stages(p, L, R)
        st = {k: oracle.stage(k) for k in STAGES}
        d1, d2, _ = oracle.process(p, L, R)
        out[name] = (L, R, n, st, d1, d2)
    return out


def _engine(eng, name, L, **kw):
    return eng.StereoEngine(L.shape[1], L.shape[0], degenerate_sets.pair_params(eng.SvParams, name), **kw)


def test_pairs_are_grouped_completely():
    assert sorted(n for g in GROUPS for n in g) == sorted(PAIRS) and len(PAIRS) == 7
    assert any(degenerate_sets.pair_params(ElasParams, n).subsampling == 1 for n in PAIRS)


@pytest.mark.parametrize("name", PAIRS)
def test_degenerate_pair_every_stage(eng, wanted, name):
    """Every stage sv_debug_get exposes, the status and the final maps against the oracle, on a keep_debug handle (one pair at a time,
    host triangulation: the engine's rule); the band pairs have triangulations without a triangle (both sides / the left side)."""
    L, R, n, st, o1, o2 = wanted[name]
    e = _engine(eng, name, L, keep_debug=True, triangulation="gpu")  # (asked for, and not honoured with keep_debug)
    try:
        q = e.query()
        assert q["gpu_triangulation"] == 0 and q["resident"] == 0 and q["chunk"] == 1
        d1, d2, status = e.process_host(L, R)
        got = {k: e.debug(k) for k in STAGES}
    finally:
        e.close()
    assert status[0] == n and n >= 3
    bad = [k for k in STAGES if got[k].size != st[k].size or not np.array_equal(got[k].view(np.uint8), st[k].view(np.uint8))]
    assert not bad, bad
    assert np.array_equal(d1[0].view(np.uint8), o1.view(np.uint8)) and np.array_equal(d2[0].view(np.uint8), o2.view(np.uint8))


@pytest.mark.parametrize("inline", [None, False])
def test_degenerate_pairs_latency_handle(eng, wanted, inline):
    """chunk = 1 (the calling thread drives the pair, or the pool does; host triangulation: the engine's rule): every pair three times on
    one handle."""
    done = 0
    for name in PAIRS:
        L, R, n, st, o1, o2 = wanted[name]
        e = _engine(eng, name, L, chunk=1, n_streams=1, n_slots=2, n_workers=2, inline=inline)
        try:
            q = e.query()
            assert q["chunk"] == 1 and q["gpu_triangulation"] == 0 and q["resident"] == 0
            for _ in range(3):
                d1, d2, status = e.process_host(L, R)
                assert status[0] == n, name
                assert np.array_equal(d1[0].view(np.uint8), o1.view(np.uint8)) and np.array_equal(d2[0].view(np.uint8), o2.view(np.uint8)), name
        finally:
            e.close()
        done += 1
    assert done == len(PAIRS)


def _ordinary_pair(h, w):
    """An ordinary pair of this size: the KITTI crop where it is large enough, else a synthetic pair."""
    K = util.case_images(util.digests()["kitti0_crop_d64"])
    if h <= K[0].shape[0] and w <= K[0].shape[1]:
        return np.ascontiguousarray(K[0][:h, :w]), np.ascontiguousarray(K[1][:h, :w])
    return util.pkg("synth").make_pair(77, h, w, 32)


@pytest.mark.parametrize("group", GROUPS, ids=lambda g: g[0])
@pytest.mark.parametrize("mode", list(BATCH_MODES))
def test_degenerate_pairs_inside_batches(eng, oracle, wanted, mode, group):
    """Batch handles (chunk 4, a ragged last chunk) with the triangulations on the host pool, on the device with the support lists resident,
    and on the device from lists the pool ordered - asserted from sv_query.  Every pair (the half-resolution one included) sits first,
    last and between ordinary pairs, and in a batch made of degenerate pairs only (row and column bands mixed where they share a handle);
    each pair equals its own oracle result, twice on the same handle.  Degenerate-only batches leave nothing to the fallback."""
    triangulation, resident, q_gpu, q_res = BATCH_MODES[mode]
    name = group[0]
    h, w = wanted[name][0].shape
    po = degenerate_sets.pair_params(ElasParams, name)
    KL, KR = _ordinary_pair(h, w)
    kn = oracle.run_stages(po, KL, KR)
    k1, k2, _ = oracle.process(po, KL, KR)
    pairs = {"K": (KL, KR, kn, k1, k2)}
    for c, nm in zip("AB", group):
        L, R, n, st, o1, o2 = wanted[nm]
        sup = st["support"].reshape(-1, 3)
        assert len(np.unique(np.stack([sup[:, 0] - sup[:, 2], sup[:, 1]], 1), axis=0)) == n, nm  # no coincident vertices: nothing for the host to take back
        pairs[c] = (L, R, n, o1, o2)
    second = "B" if len(group) > 1 else "A"
    for layout in ("AKK" + second + "KKA", "A" + second + "A" + second + "A"):
        Ls, Rs = np.stack([pairs[c][0] for c in layout]), np.stack([pairs[c][1] for c in layout])
        e = _engine(eng, name, wanted[name][0], chunk=4, n_slots=2, n_streams=2, n_workers=3, triangulation=triangulation, resident=resident)
        try:
            q = e.query()
            assert q["chunk"] == 4 and q["gpu_triangulation"] == q_gpu and q["resident"] == q_res, q
            for _ in range(2):
                d1, d2, status = e.process_host(Ls, Rs)
                for i, c in enumerate(layout):
                    _, _, wn, w1, w2 = pairs[c]
                    assert status[i] == wn, (layout, i)
                    assert np.array_equal(d1[i].view(np.uint8), w1.view(np.uint8)) and np.array_equal(d2[i].view(np.uint8), w2.view(np.uint8)), (layout, i)
            if q_gpu:
                assert e.gpu_triangulation_share() == 1.0
                if "K" not in layout:
                    assert e.gpu_triangulation_fallbacks() == 0
        finally:
            e.close()
