"""The stages that hand a value from one thread to the next through the scans and reductions of csrc/wave_ops.h and add a carry of
their own on top - k_stixel_objects, k_box_positions, k_ground_hist / k_ground_search / k_ground_pick, k_cloud_scan, k_voxel_write - on
cases built thread by thread in tests/scan_carry_cases.py: segments, medians, bins, tiles and owner bits placed on the last cell of one
thread's, wavefront's or chunk's share and on the first cell of the next.

The reference is always the numpy definition in stereo_vision.sv on the CPU and every comparison is bit for bit, doubles included (the
stages' own test modules say why).  The CPU tests assert of every case that it realises the layout it names, that the numpy model of the
kernel's carry step is the definition, and that the model with the ONE mistake the case is aimed at - a wavefront's or a thread's base
dropped, the previous chunk's carry dropped, a clamp off by one, a tie taken by the larger index - gives another output of the stage.
Two cases have nothing a rank or a base could move and are held to the first two assertions only: the voxel pattern "nothing" and the
one-tile cloud whose tile holds 0 = 0 % 5 points; both must come back empty."""
import collections
import time

import numpy as np
import pytest

import scan_carry_cases as sc
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_ground import OUTPUTS as GROUND_OUTPUTS, _bits, _gpu as _ground_gpu
from test_stixels import _raw as _stixel_raw
from test_box_positions import _same as _box_same
from test_compact_cloud import _gpu as _cloud_gpu
from test_voxel_cloud import _gpu as _voxel_gpu, _same as _voxel_same

POISON = sc.POISON


# ---------------------------------------------------------------------------------------------------------------- CPU: stixel objects

def _objects_equal(a, b):
    return a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _stixel_want(sv, c):
    d, lab = sc.stixel_map(c.q, c.top, c.bottom, c.col_step)
    st, n = sv.stixels(d, lab, col_step=c.col_step, sim_cols=c.sim_cols, min_cols=c.min_cols, **sc.STIXEL_SPEC)
    return d, lab, st, n, sv.stixel_objects(st[0], c.col_step, c.sim_cols, c.min_cols, c.capacity)


def test_stixel_cases_realise_their_layouts_and_show_their_mistakes(sv):
    cases = sc.stixel_cases()
    for c in cases.values():
        d, lab, st, n, want = _stixel_want(sv, c)
        assert d.shape == (4, (len(c.q) - 1) * c.col_step + 1) and np.array_equal(st[0], sc.stixel_layer0(c.q, c.top, c.bottom)) and np.array_equal(n, c.q >= 0), c.name
        every = sv.stixel_objects(st[0], c.col_step, c.sim_cols, c.min_cols)  # uncapped: the segments the case names, first and last column
        segs = [(int(b[0]) // c.col_step, (int(b[0]) + int(b[2]) - 1) // c.col_step) for b in every[0]]
        assert segs[:len(c.segments)] == list(c.segments) and (c.name.startswith("capacity") or len(segs) == len(c.segments)), (c.name, segs[:4])
        assert c.q_med is None or want[1][0][3] == c.q_med, (c.name, want[1][0])
        assert _objects_equal(sc.stixel_objects_model(st[0], c.col_step, c.sim_cols, c.min_cols, c.capacity), want), c.name
        assert c.aimed, c.name
        for bug in c.aimed:
            assert not _objects_equal(sc.stixel_objects_model(st[0], c.col_step, c.sim_cols, c.min_cols, c.capacity, bug), want), (c.name, bug)
    # the family holds what it was asked to hold
    assert sc.STIXEL_WIDTHS == (64, 65, 255, 256, 257, 511, 512, 513, 769, 1025) and sc.STIXEL_EDGES == (63, 127, 191, 255, 511, 767)
    for e in sc.STIXEL_EDGES:
        widths = [w for w in sc.STIXEL_WIDTHS if e + 1 < w]
        for kind in ("split", "across", "sim_joins", "sim_splits"):
            assert all("%s_%d_%d" % (kind, e, w) in cases for w in widths if kind != "split" or w - 1 - e >= 3), (kind, e)
        for kind in ("min_cols", "min_cols_less_one"):
            assert all("%s_%d_%d" % (kind, e, w) in cases for w in widths if e + 2 < w), (kind, e)
        c = cases["across_%d_%d" % (e, widths[-1])]
        assert c.q[e] >= 0 and c.q[e + 1] >= 0 and c.segments[-1][0] <= e < c.segments[-1][1]
        c = cases["split_%d_%d" % (e, widths[-1])]
        assert c.segments[-2][1] == e and c.segments[-1][0] == e + 1
        assert len(cases["min_cols_%d_%d" % (e, widths[-1])].segments) == 2 and len(cases["min_cols_less_one_%d_%d" % (e, widths[-1])].segments) == 1
    assert all(cases["tail_%d" % w].segments[-1] == (w - 4, w - 1) for w in sc.STIXEL_WIDTHS)
    assert all("whole_%d" % w in cases for w in (257, 513, 1025)) and cases["chunk_0_to_2"].segments == ((200, 600),) and (cases["chunk_0_to_2"].q[256:512] == 100).all()
    for n in sc.STIXEL_LENGTHS:
        for kind in sc.STIXEL_MULTISETS:
            assert ("median_%s_%d" % (kind, n) in cases) == (not (kind == "median_at_63" and n < 64) and not (kind == "median_at_64" and n < 65))
    c = cases["median_full_range_129"]
    assert c.q.min() == -1 and sorted(set(c.q[c.q >= 0])) == [0, 1000, 4095]
    for at in (63, 64):
        c = cases["median_median_at_%d_129" % at]
        assert np.nonzero(c.q == 400)[0].tolist() == [5 + at] and c.q_med == 400
    q = sc.stixel_short_segments()
    assert len(q) == 513 and all(q[2 * k] == q[2 * k + 1] and abs(q[2 * k + 2] - q[2 * k]) in (7, 14) for k in range(255))  # sim_cols is 2
    assert [cases["capacity_%d" % cap].capacity for cap in sc.STIXEL_CAPACITIES] == [0, 1, 50, 128, 129, 200, 255, 256] and sc.STIXEL_SHORT_TOTAL == 256
    assert any(c.col_step == 3 for c in cases.values())


# ---------------------------------------------------------------------------------------------------------------- CPU: boxes

def _box_hist(sv, d, disparity, rows=1):
    q, valid, _ = sv.box_quantise(d[:rows, :-1], disparity)
    return np.bincount(q[valid], minlength=sc.BOX_BINS)


def test_box_median_cases_realise_their_layouts_and_show_their_mistakes(sv):
    cases = sc.box_median_cases()
    names = {c.name for c in cases}
    for c in cases:
        d, box = sc.box_median_map(c.bins, c.disparity)
        _, stat = sv.box_positions(d, [box], Q=sc.BOX_Q, select="valid", disparity=c.disparity)
        hist = _box_hist(sv, d, c.disparity)
        assert np.array_equal(hist, sc.box_histogram(c.bins)) and stat[0].tolist() == [sc.BOX_MEDIAN_WIDTH, c.n_valid, c.median, c.n_valid], (c.name, stat[0])
        assert sc.box_median_model(hist) == (c.n_valid, [c.median]), c.name
        assert c.aimed and all(sc.box_median_model(hist, bug) != (c.n_valid, [c.median]) for bug in c.aimed), c.name
        m, kind, top = c.median, c.name.split("_", 2)[2], sc.BOX_TOP[c.disparity]
        # which kinds must show which mistakes
        if kind.startswith("even") or (kind == "two" and m < top):
            assert "upper_median" in c.aimed and c.n_valid % 2 == 0, c.name
            upper = int(np.sort(c.bins)[c.n_valid // 2])
            assert kind == "two" or upper // sc.BOX_PER != m // sc.BOX_PER, c.name
            assert kind != "even_next_wave" or (upper // 1024 != m // 1024 and "wave_base" in c.aimed), c.name
        if kind in ("odd", "even_next_thread", "even_next_wave") and m >= sc.BOX_PER and m < top:
            assert "thread_base" in c.aimed, c.name
        if kind in ("odd", "even_next_thread", "even_next_wave") and m >= 1024 and m < top:
            assert "wave_base" in c.aimed, c.name
        if kind == "one_bin":
            assert set(c.bins.tolist()) == {m} and c.aimed == ("total_without_wave_%d" % (m // 1024),), c.name
    for disparity, medians in sc.BOX_MEDIANS.items():
        for m in medians:
            for kind in sc.BOX_KINDS:
                expected = not (kind.startswith("even") and m == sc.BOX_TOP[disparity]) and not (kind == "even_next_wave" and (m // 1024 + 1) * 1024 > sc.BOX_TOP[disparity]) \
                    and not (kind == "even_next_thread" and (m // 16 + 1) * 16 + 3 > sc.BOX_TOP[disparity])
                assert ("%s_%d_%s" % (disparity, m, kind) in names) == expected, (disparity, m, kind)
    assert sc.BOX_MEDIANS == {"d1": (0, 1, 15, 16, 17, 1023, 1024, 4079, 4080, 4095), "dmap": (1, 15, 16, 255)}
    # the last bin of a thread's 16 with the next pixel in the next thread: a thread that also takes "my bins start AT the rank" answers too
    assert all("select_le" in c.aimed for c in cases if c.name in ("d1_15_even_next_thread", "d1_1023_even_next_thread", "d1_4079_even_next_thread", "dmap_15_even_next_thread"))
    for disparity, medians in sc.BOX_BAND_MEDIANS.items():
        for m in medians:
            bins = sc.box_band_bins(m)
            d, box = sc.box_median_map(bins, disparity)
            hist = _box_hist(sv, d, disparity)
            assert (m + 1) % sc.BOX_PER == 0 and hist[m + 1] == 3 and hist[m - 1] == 2  # the band 1 reaches the next thread's first bin, by exactly one bin
            for band, n_sel in sc.BOX_BAND_SELECTED.items():
                _, stat = sv.box_positions(d, [box], Q=sc.BOX_Q, select="near", disparity=disparity, band=band)
                assert stat[0].tolist() == [sc.BOX_MEDIAN_WIDTH, 13, m, n_sel] and sc.box_near_model(hist, m, band) == n_sel
                assert sc.box_near_model(hist, m, band, "band_lt") != n_sel


def _sum_selection(sv, d, box, select):
    w, r = box[2], box[3]
    q, valid, dd = sv.box_quantise(d, "d1")
    P = sv._box_points(dd, sc.BOX_Q, None, None)[:r, :w]
    pos, stat = sv.box_positions(d, [box], Q=sc.BOX_Q, select=select, disparity="d1", band=4)
    sel = valid[:r, :w] if select == "valid" else valid[:r, :w] & (np.abs(q[:r, :w] - stat[0][2]) <= 4)
    return P, sel, pos[0], stat[0]


def test_box_sum_cases_realise_their_layouts_and_show_their_mistakes(sv):
    for w in sc.BOX_SUM_WIDTHS:
        for r in sc.BOX_SUM_ROWS:
            for where in sc.BOX_SUM_WHERE:
                d, box = sc.box_sum_map(w, r, where)
                assert d.shape == (r + 1, w + 1) and box == (0, 0, w, r)
                for select in ("valid", "near"):
                    P, sel, pos, stat = _sum_selection(sv, d, box, select)
                    cols = np.nonzero(sel.any(0))[0].tolist()
                    assert cols == {"last": [w - 1], "first": [0], "every": list(range(w))}[where] and stat[3] == sel.sum() > 0 and stat[0] == w * r, (w, r, where, select)
                    total = sc.box_sum_model(P, sel)
                    assert np.array_equal((total / np.float64(stat[3])).view(np.int64), pos.view(np.int64)), (w, r, where, select)
                    caught = [bug for bug in sc.BOX_SUM_BUGS if not np.array_equal(sc.box_sum_model(P, sel, bug).view(np.int64), total.view(np.int64))]
                    must = {"last": ["last_column"], "first": ["first_column"] + (["chunk_carry"] if w > 256 else []),
                            "every": ["last_column", "first_column"] + (["chunk_carry"] if w > 256 else []) + (["right_to_left"] if w >= 255 else [])}[where]
                    assert all(bug in caught for bug in must), (w, r, where, select, caught)
    assert sc.BOX_SUM_WIDTHS == (1, 2, 255, 256, 257, 511, 512, 513) and sc.BOX_SUM_ROWS == (1, 3)


# ---------------------------------------------------------------------------------------------------------------- CPU: ground

def _ground_cases():
    return [c for n in sc.GROUND_BINS for c in sc.ground_boundary_cases(n)] + sc.ground_tie_cases()


def test_ground_cases_realise_their_layouts_and_show_their_mistakes(sv):
    cases = {c.name: c for c in _ground_cases()}
    for c in cases.values():
        want = sv.ground(c.d, **dict(c.spec))
        rec = want["ground"].tolist()
        assert c.d.shape[0] <= 8 or c.d.shape[1] == 1, c.name
        assert list(sc.ground_model(sv, c.d, c.spec)) == rec, (c.name, rec)
        assert c.must or c.name == "all_invalid", c.name
        for bug in c.must:
            assert list(sc.ground_model(sv, c.d, c.spec, bug)) != rec, (c.name, bug, rec)
    assert sc.GROUND_BINS == (8, 255, 256, 257, 511, 512, 513, 4081, 4095, 4096)
    for n_bins in sc.GROUND_BINS:
        per = (n_bins + 255) // 256
        edges = sc.ground_boundaries(n_bins)
        assert edges["thread_1"] == per and edges["last_bin"] == n_bins - 1 and edges["last_thread"] == (n_bins - 1) // per * per
        assert all(edges.get("wave_%d" % k) == 64 * k * per for k in (1, 2, 3) if 64 * k * per < n_bins)
        for name, j in edges.items():
            if j == n_bins - 1 and name != "last_bin":
                continue
            c = cases["bins_%d_%s" % (n_bins, name)]
            vdisp, (vh, qb, S, n_valid) = sv.v_disparity(c.d, n_bins), sv.ground(c.d, **dict(c.spec))["ground"].tolist()
            assert vdisp[1, j - 1] == 5 and vdisp[1, j] == 4 and vdisp[1].sum() == 11 and n_valid == 12, c.name  # the mass on both sides, on the bottom row
            assert (vh, S) == (0, 9) and max(qb - 1, 0) < j < qb + 2, (c.name, qb)  # the winner's window lo .. hi - 1 straddles j - 1 | j
            if name == "last_bin":
                assert np.isinf(c.d[1]).sum() == 2 and (c.d[1] == np.float32(1e6)).sum() == 1
                alone = cases["bins_%d_last_bin_alone" % n_bins]
                assert sv.ground(alone.d, **dict(alone.spec))["ground"].tolist() == [0, n_bins - 1, 5, 12] and alone.spec["tol"] == 0
    # the ties: the smallest vh, then the smallest qb
    assert sv.ground(cases["all_invalid"].d, **dict(cases["all_invalid"].spec))["ground"].tolist() == [-3, 2, 0, 0]
    for n_qb, star in ((255, 64), (256, 64), (257, 64), (257, 256), (600, 64), (600, 256), (600, 520)):
        c = cases["tie_qb_%d_at_%d" % (n_qb, star)]
        assert len(range(1, c.spec["n_bins"])) == n_qb and sv.ground(c.d, **dict(c.spec))["ground"].tolist() == [-2, star - 1, 3, 3]  # iq = star - 2, star - 1 and star tie
    for n_vh in (255, 256, 257, 600):
        c = cases["tie_vh_%d" % n_vh]
        assert len(range(c.spec["vh_lo"], 1)) == n_vh and sv.ground(c.d, **dict(c.spec))["ground"].tolist() == [1 - n_vh, 4, 3, 3]
    assert sv.ground(cases["second_trip_by_one"].d, **dict(cases["second_trip_by_one"].spec))["ground"].tolist() == [0, 300, 4, 7]  # iq 299 over iq 39, 4 over 3
    assert sv.ground(cases["wave_3_by_one"].d, **dict(cases["wave_3_by_one"].spec))["ground"].tolist() == [0, 200, 4, 7]  # iq 199 over iq 9
    for n_vh in (257, 600):
        c = cases["pick_trip_by_one_%d" % n_vh]
        assert sv.ground(c.d, **dict(c.spec))["ground"].tolist() == [0, 100, 4, 4]  # ivh = n_vh - 1, past the first 256
    for H in (257, 513):
        c = cases["rows_%d" % H]
        assert c.d.shape == (H, 1) and sv.ground(c.d, **dict(c.spec))["ground"][3] == (c.d > 0).sum() > (c.d[:256] > 0).sum() > 0


# ---------------------------------------------------------------------------------------------------------------- CPU: cloud and voxels

CLOUD_TILE = 1024  # the GPU tests assert that the library's tile is this one
CLOUD_EMPTY = ("index_mod_5_1",)


def _cloud_capacities(c, total):
    """The total, the total minus 1, and - past 256 tiles - the offset of tile 256 exactly."""
    counts = np.bincount(np.nonzero(sc.cloud_keep(c))[0] // c.tile, minlength=257)
    caps = {total, max(total - 1, 0)} | ({int(counts[:256].sum())} if c.n_visited > 256 * c.tile and c.pattern in ("index_mod_5", "full") else set())
    return sorted(caps)


def _cloud_must(c):
    n = -(-c.n_visited // c.tile)
    return {"last_tile": ["hi_clamp"], "tile_0": ["total_without_wave_0"], "index_mod_5": ["total_without_wave_0"] + (["thread_base"] if n > 2 else []) + (["wave_base"] if n > 64 else []),
            "full": ["hi_clamp"] + (["thread_base"] if n > 1 else []) + (["wave_base"] if n > 64 else [])}[c.pattern]


def test_cloud_cases_realise_their_layouts_and_show_their_mistakes(sv):
    cases = sc.cloud_cases(CLOUD_TILE)
    assert {(-(-c.n_visited // c.tile)) for c in cases if c.step == 1 and c.n_visited % c.tile == 0} == set(sc.CLOUD_TILES)
    assert {c.n_visited for c in cases} >= {256 * 1024 - 1, 256 * 1024 + 1, 512 * 1024 - 1, 512 * 1024 + 1} and sum(c.step == 2 for c in cases) == 2
    for c in cases:
        d = sc.cloud_map(c)
        assert d.size <= 600000 and -(-d.shape[1] // c.step) == c.n_visited
        _, _, index = sv.compact_cloud(d, sc.CLOUD_Q, step=c.step, **sc.CLOUD_CROP)
        keep = sc.cloud_keep(c)
        counts = np.bincount(np.nonzero(keep)[0] // c.tile, minlength=-(-c.n_visited // c.tile))
        assert np.array_equal(index, np.nonzero(keep)[0] * c.step), c.name
        n = len(counts)
        want = {"last_tile": [0] * (n - 1) + [counts[-1]], "tile_0": [c.tile] + [0] * (n - 1), "index_mod_5": [min(t % 5, c.n_visited - t * c.tile) for t in range(n)], "full": counts.tolist()}[c.pattern]
        assert counts.tolist() == want and (c.pattern != "last_tile" or counts[-1] > 0), c.name
        total = len(index)
        rows, count = sc.cloud_rows_model(c, total)
        assert count == total and np.array_equal(rows, index), c.name
        if c.name in CLOUD_EMPTY:
            assert total == 0
            continue
        for bug in _cloud_must(c):
            rows, count = sc.cloud_rows_model(c, total, bug)
            assert count != total or not np.array_equal(rows, index), (c.name, bug)
        cap = total - 1  # the row at the capacity stays the caller's
        rows, count = sc.cloud_rows_model(c, cap)
        assert count == total and np.array_equal(rows, index[:cap])
        assert len(sc.cloud_rows_model(c, cap, "capacity_plus_one")[0]) == total


def test_voxel_cases_realise_their_layouts_and_show_their_mistakes(sv):
    for tiles in (1, 2):
        for pattern in sc.VOXEL_PATTERNS:
            d = sc.voxel_rank_map(pattern, tiles, CLOUD_TILE)
            keep = sc.voxel_owner_bits(pattern, tiles, CLOUD_TILE)
            lanes = keep.reshape(tiles, 64, 16)
            assert {"lane_63": lanes[:, 63].all() and not lanes[:, :63].any(), "lane_0": lanes[:, 0].all() and not lanes[:, 1:].any(), "bit_per_lane": (lanes.sum(2) == 1).all(),
                    "all": keep.all(), "nothing": not keep.any()}[pattern]
            xyz, _, cell, n, first, count = sv.voxel_cloud(d, sc.CLOUD_Q, dtype="f64", **sc.VOXEL_RANK_GRID)
            where = np.nonzero(keep)[0]
            assert count == keep.sum() and np.array_equal(first, where) and (n == 1).all() and np.array_equal(cell, np.repeat(where[:, None], 3, 1))  # a voxel of its own
            assert np.array_equal(sc.voxel_rows_model(keep, CLOUD_TILE), first)
            caught = [bug for bug in sc.VOXEL_BUGS if not np.array_equal(sc.voxel_rows_model(keep, CLOUD_TILE, bug), first)]
            must = [] if pattern == "nothing" else ["inclusive"] + (["lane_base"] if pattern in ("bit_per_lane", "all") else []) + (["tile_offset"] if tiles == 2 else [])
            assert caught == [bug for bug in sc.VOXEL_BUGS if bug in must], (tiles, pattern, caught)


# ---------------------------------------------------------------------------------------------------------------- GPU: stixel objects

def _stixel_run(sv, eng, cases, boxes=True, info=True):
    """The C entry on caller-owned, POISON-filled buffers for cases that share a width and a spec, one frame each: counts uncapped, the
    first min(count, capacity) rows the definition's, every row at and past the capacity - and a tail behind the buffer - untouched."""
    import torch
    c0 = cases[0]
    assert all((len(c.q), c.col_step, c.sim_cols, c.min_cols, c.capacity) == (len(c0.q), c0.col_step, c0.sim_cols, c0.min_cols, c0.capacity) for c in cases)
    wants = [_stixel_want(sv, c) for c in cases]
    d, lab = np.stack([w[0] for w in wants]), np.stack([w[1] for w in wants])
    B, cap, Wv = len(cases), c0.capacity, len(c0.q)
    spec = eng.stixel_spec(col_step=c0.col_step, sim_cols=c0.sim_cols, min_cols=c0.min_cols, **sc.STIXEL_SPEC)
    fill = lambda *shape: torch.full(shape, POISON, dtype=torch.int32, device="cuda")  # noqa: E731
    out = {"stixels": fill(B, 1, Wv, 4), "n_stixels": fill(B, Wv), "boxes": fill(B * cap * 4 + 8), "info": fill(B * cap * 4 + 8), "counts": fill(B)}
    _stixel_raw(eng, _cuda(d), _cuda(lab), spec, cap, out["stixels"], out["n_stixels"], out["boxes"] if boxes else None, out["info"] if info else None, out["counts"])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for b, (c, (_, _, st, n, (bx, nf, count))) in enumerate(zip(cases, wants)):
        assert got["counts"][b] == count and _bits(got["stixels"][b], st) and _bits(got["n_stixels"][b], n), (c.name, got["counts"][b], count)
        for key, want, asked in (("boxes", bx, boxes), ("info", nf, info)):
            rows = got[key][4 * cap * b:4 * cap * (b + 1)].reshape(cap, 4)
            k = len(want) if asked else 0
            assert k == (min(count, cap) if asked else 0) and _bits(rows[:k], want[:k]), (c.name, key, rows[:k].tolist()[:6], want.tolist()[:6])
            assert (rows[k:] == POISON).all(), (c.name, key)
    assert (got["boxes"][4 * cap * B:] == POISON).all() and (got["info"][4 * cap * B:] == POISON).all()


def _stixel_groups(cases):
    groups = collections.OrderedDict()
    for c in cases:
        groups.setdefault((len(c.q), c.col_step, c.sim_cols, c.min_cols, c.capacity), []).append(c)
    return list(groups.values())


@pytest.mark.gpu
@pytest.mark.parametrize("width", sc.STIXEL_WIDTHS)
def test_stixel_segments_at_wavefront_and_chunk_edges(sv, eng, width):
    t0 = time.time()
    cases = sc.stixel_edge_cases(width)
    if width == 257:
        cases = cases + [c._replace(col_step=3) for c in cases]
    for group in _stixel_groups(cases):
        _stixel_run(sv, eng, group)
    print("stixel edges, width %d: %d cases, %.2f s" % (width, len(cases), time.time() - t0))


@pytest.mark.gpu
def test_stixel_segments_over_several_chunks_and_their_medians(sv, eng):
    t0 = time.time()
    cases = sc.stixel_long_cases() + sc.stixel_median_cases()
    for group in _stixel_groups(cases):
        _stixel_run(sv, eng, group)
    print("stixel long segments and medians: %d cases, %.2f s" % (len(cases), time.time() - t0))


@pytest.mark.gpu
def test_stixel_capacity_inside_and_at_the_end_of_a_chunk(sv, eng):
    t0 = time.time()
    cases = sc.stixel_capacity_cases()
    for c in cases:
        _stixel_run(sv, eng, [c])
    for c in cases[1:]:  # the null-output forms: boxes only, info only
        _stixel_run(sv, eng, [c], info=False)
        _stixel_run(sv, eng, [c], boxes=False)
    print("stixel capacities: %d cases x 3 forms, %.2f s" % (len(cases), time.time() - t0))


# ---------------------------------------------------------------------------------------------------------------- GPU: boxes

def _box_check(sv, eng, d, boxes, what, **kw):
    """GPU == definition on a batch of maps with one box each: the doubles bit for bit (NaN where nothing is selected), stat exactly."""
    boxes = np.asarray(boxes, np.int32).reshape(len(d), 1, 4)
    pos, stat = eng.box_positions_from_disparity(_cuda(d), sc.BOX_Q, boxes, **kw)
    want_pos, want_stat = sv.box_positions(d, boxes, Q=sc.BOX_Q, **kw)
    got_pos, got_stat = pos.cpu().numpy(), stat.cpu().numpy()
    for b in range(len(d)):
        assert got_stat[b].tolist() == want_stat[b].tolist(), (what[b], kw, got_stat[b].tolist(), want_stat[b].tolist())
        assert _box_same(got_pos[b], want_pos[b]), (what[b], kw, got_pos[b].tolist(), want_pos[b].tolist())
    return want_stat


@pytest.mark.gpu
@pytest.mark.parametrize("disparity", ["d1", "dmap"])
def test_box_median_on_thread_and_wavefront_edges(sv, eng, disparity):
    t0 = time.time()
    cases = [c for c in sc.box_median_cases() if c.disparity == disparity]
    maps = [sc.box_median_map(c.bins, disparity) for c in cases]
    d, boxes, names = np.stack([m[0] for m in maps]), [m[1] for m in maps], [c.name for c in cases]
    for kw in (dict(select="valid"), dict(select="near", band=0), dict(select="near", band=1), dict(select="near", band=4)):
        stat = _box_check(sv, eng, d, boxes, names, disparity=disparity, **kw)
        assert stat[:, 0, 2].tolist() == [c.median for c in cases] and stat[:, 0, 1].tolist() == [c.n_valid for c in cases]
    medians = sc.BOX_BAND_MEDIANS[disparity]
    maps = [sc.box_median_map(sc.box_band_bins(m), disparity) for m in medians]
    for band, n_sel in sc.BOX_BAND_SELECTED.items():
        stat = _box_check(sv, eng, np.stack([m[0] for m in maps]), [m[1] for m in maps], ["band_%d" % m for m in medians], disparity=disparity, select="near", band=band)
        assert stat[:, 0, 3].tolist() == [n_sel] * len(medians) and stat[:, 0, 2].tolist() == list(medians)
    print("box medians, %s: %d + %d cases, %.2f s" % (disparity, len(cases), len(medians), time.time() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("width", sc.BOX_SUM_WIDTHS)
def test_box_sums_over_chunks_of_columns(sv, eng, width):
    t0 = time.time()
    for rows in sc.BOX_SUM_ROWS:
        maps = [sc.box_sum_map(width, rows, where) for where in sc.BOX_SUM_WHERE]
        d, boxes = np.stack([m[0] for m in maps]), [m[1] for m in maps]
        what = ["%s_%d_%d" % (where, width, rows) for where in sc.BOX_SUM_WHERE]
        for kw in (dict(disparity="d1", select="valid"), dict(disparity="d1", select="near", band=4), dict(disparity="dmap", select="valid"), dict(disparity="dmap", select="near", band=4)):
            stat = _box_check(sv, eng, d, boxes, what, **kw)
            assert (stat[:, 0, 3] > 0).all() and stat[2, 0, 1] == width * rows
    print("box sums, width %d: 6 cases x 4 forms, %.2f s" % (width, time.time() - t0))


# ---------------------------------------------------------------------------------------------------------------- GPU: ground

def _ground_check(sv, eng, cases, monkeypatch):
    """Cases of one shape and spec as one batch, with the histogram's aggregation and without it: all five outputs are the definition's."""
    d = np.stack([c.d for c in cases])
    spec = dict(cases[0].spec)
    wants = [sv.ground(c.d, **dict(spec)) for c in cases]
    for hist in ("default", "plain"):
        if hist == "plain":
            monkeypatch.setenv("SV_GROUND_HIST", "plain")
        else:
            monkeypatch.delenv("SV_GROUND_HIST", raising=False)
        got = _ground_gpu(eng, d, **spec)
        for b, (c, want) in enumerate(zip(cases, wants)):
            assert got["ground"][b].tolist() == want["ground"].tolist(), (c.name, hist, got["ground"][b].tolist(), want["ground"].tolist())
            assert all(_bits(got[k][b], want[k]) for k in GROUND_OUTPUTS), (c.name, hist, [k for k in GROUND_OUTPUTS if not _bits(got[k][b], want[k])])
        assert _bits(got["vdisp"], sv.v_disparity(d, spec["n_bins"]))
    monkeypatch.delenv("SV_GROUND_HIST", raising=False)


def _ground_groups(cases):
    groups = collections.OrderedDict()
    for c in cases:
        groups.setdefault((c.d.shape, tuple(sorted(c.spec.items()))), []).append(c)
    return list(groups.values())


@pytest.mark.gpu
@pytest.mark.parametrize("n_bins", sc.GROUND_BINS)
def test_ground_bin_scan_at_thread_and_wavefront_edges(sv, eng, n_bins, monkeypatch):
    t0 = time.time()
    cases = sc.ground_boundary_cases(n_bins)
    for group in _ground_groups(cases):
        _ground_check(sv, eng, group, monkeypatch)
    print("ground bin scan, %d bins: %d cases x 2 histogram forms, %.2f s" % (n_bins, len(cases), time.time() - t0))


@pytest.mark.gpu
def test_ground_arg_max_ties_and_trips(sv, eng, monkeypatch):
    t0 = time.time()
    cases = sc.ground_tie_cases()
    for group in _ground_groups(cases):
        _ground_check(sv, eng, group, monkeypatch)
    print("ground arg-max: %d cases x 2 histogram forms, %.2f s" % (len(cases), time.time() - t0))


# ---------------------------------------------------------------------------------------------------------------- GPU: cloud and voxels

@pytest.mark.gpu
@pytest.mark.parametrize("n_tiles", sc.CLOUD_TILES)
def test_cloud_tile_scan(sv, eng, n_tiles):
    """counts, index_out, xyz and the colours against compact_cloud: every pattern at the total, the total minus 1 and, past 256 tiles,
    the offset of tile 256 as the capacity; the cases one pixel short of and past 256 and 512 tiles and the step-2 form ride with 256,
    512 and 257."""
    t0 = time.time()
    assert eng.cloud_tile() == CLOUD_TILE
    cases = [c for c in sc.cloud_cases(CLOUD_TILE) if {"_%d" % n_tiles, "_%d-1" % n_tiles, "_%d+1" % n_tiles, "_%d_step2" % n_tiles} & {c.name[len(c.pattern):]}]
    assert len(cases) == 4 + 4 * (n_tiles in (256, 512)) + 2 * (n_tiles == 257)
    for c in cases:
        d = sc.cloud_map(c)
        colors = np.random.default_rng(c.n_visited).integers(0, 256, d.shape + (4,), dtype=np.uint8)
        for dtype in ("f32", "f64") if c.pattern != "full" or n_tiles <= 2 else ("f32",):
            wx, wc, wi = sv.compact_cloud(d, sc.CLOUD_Q, step=c.step, dtype=dtype, colors=colors, **sc.CLOUD_CROP)
            assert np.array_equal(wi, np.nonzero(sc.cloud_keep(c))[0] * c.step)
            for cap in _cloud_capacities(c, len(wi)):
                got, counts = _cloud_gpu(eng, d, sc.CLOUD_Q, colors, step=c.step, dtype=dtype, capacity=cap, **sc.CLOUD_CROP)
                gx, gc, gi = got[0]
                assert counts.tolist() == [len(wi)], (c.name, dtype, cap, counts.tolist(), len(wi))
                assert _bits(gi, wi[:cap]) and _bits(gx, wx[:cap]) and _bits(gc, wc[:cap]), (c.name, dtype, cap, gi[:8].tolist(), wi[:8].tolist())
    print("cloud tile scan, %d tiles: %d cases, %.2f s" % (n_tiles, len(cases), time.time() - t0))


@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [1, 2])
def test_voxel_row_ranks(sv, eng, tiles):
    """Every kept pixel the owner of a voxel of its own: the rows against voxel_cloud with the capacity at the total, and one row short of
    it - where the frame reports -1."""
    t0 = time.time()
    assert eng.cloud_tile() == CLOUD_TILE
    for pattern in sc.VOXEL_PATTERNS:
        d = sc.voxel_rank_map(pattern, tiles, CLOUD_TILE)
        colors = np.random.default_rng(tiles).integers(0, 256, d.shape + (4,), dtype=np.uint8)
        total = int(sc.voxel_owner_bits(pattern, tiles, CLOUD_TILE).sum())
        for dtype in ("f32", "f64"):
            for cap in sorted({max(total, 1), max(total - 1, 1)}):
                want = sv.voxel_cloud(d, sc.CLOUD_Q, colors=colors, dtype=dtype, capacity=cap, **sc.VOXEL_RANK_GRID)
                got, counts = _voxel_gpu(eng, d, sc.CLOUD_Q, colors=colors, dtype=dtype, capacity=cap, **sc.VOXEL_RANK_GRID)
                assert want[5] == (total if cap >= total else -1) and counts.tolist() == [want[5]], (pattern, dtype, cap, counts.tolist())
                assert want[5] < 0 or _voxel_same(got[0], want), (pattern, dtype, cap)
    print("voxel row ranks, %d tile(s): %d cases, %.2f s" % (tiles, len(sc.VOXEL_PATTERNS), time.time() - t0))
