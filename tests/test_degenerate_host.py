"""CPU: the host stage's triangulation (csrc/host_stage.cpp) on the structured sets of tests/degenerate_sets.py - wholly collinear
sets, collinear halves, fans, strips, complete lattices, co-circular quadruples at the extremes of the coordinate box - against the
oracle restatement.  Tolerance 0; no set is left out; each test asserts how many it ran."""
import numpy as np
import pytest

import degenerate_sets
import util

N_SETS, N_COLLINEAR = 592, 100


@pytest.fixture(scope="module")
def eng():
    util.pkg("build").build()
    return util.pkg("engine")


@pytest.fixture(scope="module")
def corpus(oracle):
    """[(name, xy, the oracle's triangle list)]"""
    return [(name, xy, oracle.delaunay(xy.astype(np.float32))) for name, xy in degenerate_sets.sets()]


def test_corpus_is_what_the_other_levels_count(corpus):
    names = [c[0] for c in corpus]
    assert len(names) == len(set(names)) == N_SETS
    empty = [name for name, xy, want in corpus if degenerate_sets.is_collinear(xy)]
    assert len(empty) == N_COLLINEAR and all(len(want) == 0 for name, xy, want in corpus if name in set(empty))
    for name, xy, _ in corpus:
        assert xy.dtype == np.int32 and xy.shape[1] == 2 and len(xy) >= 3, name
        assert xy[:, 0].min() >= degenerate_sets.X_MIN and xy[:, 1].min() >= 0 and xy.max() < 32768, name
    for depth, (w, h) in enumerate(degenerate_sets.CUT_LATTICES, 1):
        assert degenerate_sets.cut_depth(w * h, degenerate_sets.CUT_SUB_MAX) == depth


def test_host_delaunay_structured_sets(eng, corpus):
    done = 0
    for name, xy, want in corpus:
        got = eng.host_delaunay(xy)
        assert got.shape == want.shape and np.array_equal(got, want), name
        done += 1
    assert done == N_SETS


@pytest.mark.parametrize("depth,delay_us", [(1, 0), (1, 2000), (2, 0), (2, 2000)])
def test_host_delaunay_split_structured_sets(eng, corpus, depth, delay_us):
    """sv_host_delaunay_split (depth 1) / sv_host_delaunay_par: halves and quarters on other threads, also when the helper comes late
    (every 5th set: the delay is per triangulation)."""
    done = 0
    for i, (name, xy, want) in enumerate(corpus):
        got = eng.host_delaunay(xy, split=True, depth=depth, helper_delay_us=delay_us if i % 5 == 0 else 0)
        assert got.shape == want.shape and np.array_equal(got, want), name
        done += 1
    assert done == N_SETS


def test_host_delaunay_split_entry_point(eng, corpus):
    """sv_host_delaunay_split itself (the C entry point test_host_delaunay_split_structured_sets reaches through sv_host_delaunay_par)."""
    import ctypes
    L = eng.lib()
    L.sv_host_delaunay_split.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.sv_host_delaunay_split.restype = ctypes.c_int
    done = 0
    for i, (name, xy, want) in enumerate(corpus):
        out = np.empty((2 * len(xy) + 8, 3), np.int32)
        nt = L.sv_host_delaunay_split(xy.ctypes.data, len(xy), out.ctypes.data, 2 * len(xy) + 8, 1500 if i % 9 == 0 else 0)
        assert nt == len(want) and np.array_equal(out[:nt], want), name
        done += 1
    assert done == N_SETS


def test_host_kd_order_structured_sets(eng, corpus):
    """The preparation (sort, duplicate scan, alternating cuts) against a plain restatement: the distinct points in k-d order.  Which of
    several coincident vertices survives is the reference's quicksort's business (covered through the triangle lists above): here the
    survivors' coordinates and that every id is a vertex of its point."""
    done = 0
    for name, xy, _ in corpus:
        ids = eng.host_kd_order(xy)
        want = degenerate_sets.kd_order_coordinates(xy)
        assert len(ids) == len(want) and len(set(ids.tolist())) == len(ids) and np.array_equal(xy[ids], want), name
        done += 1
    assert done == N_SETS


def test_cut_path_expectations(corpus):
    """What tests/test_degenerate_sets.py expects of the cut path on the device (CUT_EXPECT), recounted here from the corpus."""
    import test_degenerate_sets as t
    for sub_max, (want_refused, want_depths) in t.CUT_EXPECT.items():
        refused, depths = 0, {}
        for name, xy, _ in corpus:
            if len(xy) <= sub_max:
                continue
            c = degenerate_sets.cut_depth(len(np.unique(xy, axis=0)), sub_max)
            if c > 6:
                refused += 1
            else:
                depths[c] = depths.get(c, 0) + 1
        assert (refused, depths) == (want_refused, want_depths), sub_max
