"""The stages that combine runs of equal keys inside a wavefront before they issue atomics - k_top_view, k_occupancy_evidence,
k_voxel_insert (wave_run / wave_run_scan of csrc/wave_ops.h), k_ground_hist (its own ladder, issued from the run's head) - on wavefront
layouts built lane by lane, and k_cloud_write's ranks (lanes_below) on hand-placed keep patterns.  The layouts come from
tests/wave_run_cases.py: runs that end at lane 63, start at lane 0, straddle a wavefront's or a workgroup's edge, are cut by a dead lane
or by the row's end.  The CPU tests assert that every map realises the layout it was built from.

The reference is always the numpy definition in stereo_vision.sv on the CPU and every comparison is bit for bit (the stages' own test
modules say why: integers behind double arithmetic in a stated order).  The debug counters are compared with ==: the number of atomics
a stage issues is a function of the per-lane keys and the split into 64 lanes, which expected_runs() computes from the keys that the
definition's arithmetic gives for the map."""
import numpy as np
import pytest

import wave_run_cases as wc
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_occupancy import OUTPUTS as OCC_OUTPUTS, _bits, _gpu as _occ_gpu, _want as _occ_want
from test_voxel_cloud import _counters as _voxel_counters, _gpu as _voxel_gpu, _same as _voxel_same
from test_ground import OUTPUTS as GROUND_OUTPUTS, _gpu as _ground_gpu
from test_compact_cloud import _gpu as _cloud_gpu

A, B, C, DEAD = wc.A, wc.B, wc.C, wc.DEAD


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_the_patterns_are_what_the_issue_asks_for():
    p = wc.PATTERNS
    assert all(len(v) == 64 for v in p.values()) and all(DEAD <= k < wc.N_KEYS for v in p.values() for k in v)
    assert len(set(p["one_run"])) == 1 and len(set(p["all_distinct"])) == 64 and p["alternating"][:4] == [A, B, A, B]
    assert p["halves"][31:33] == [A, B] and p["thirty_one_thirty_three"][30:32] == [A, B] and p["thirty_one_thirty_three"][31:33] == [B, B]
    assert [n for _, _, n, _ in wc.expected_runs(p["ramp"], 64)] == list(range(1, 11)) + [9]
    assert p["tail_at_62"][62:] == [A, B] and p["head_at_1"][:2] == [B, A] and p["last_two"] == [DEAD] * 62 + [A, A]
    assert p["hole"].count(DEAD) == 3 and set(p["hole"]) == {A, DEAD} and len(wc.expected_runs(p["hole"], 64)) == 3
    assert set(p["holes_only"]) == {DEAD} and p["lone_63"] == [DEAD] * 63 + [A] and p["lone_0"] == [A] + [DEAD] * 63
    assert p["straddle_lo"][63] == p["straddle_hi"][0] == A and p["top_key"][0] == wc.TOP == wc.N_KEYS - 1
    assert {n for g in wc.GROUPS for n in g[:5]} == set(p) and all(len(g) == 6 for g in wc.GROUPS) and len(wc.GROUPS) == 9
    # lanes 255 | 256 of a row: the straddle, one key on both sides of the edge, and the two lone lanes
    rows = wc.row_keys(321)
    assert rows.shape == (2, 9, 321) and np.array_equal(rows[1], rows[0][:, ::-1]) and not np.array_equal(rows[1], rows[0])
    assert wc.GROUPS[0][3:5] == ("straddle_lo", "straddle_hi") and rows[0, 0, 255] == rows[0, 0, 256] == A and rows[0, 0, 254] == A and rows[0, 0, 257] == A
    assert rows[0, 1, 192:321].tolist() == [A] * 129 and rows[0, 3, 254:258].tolist() == [DEAD, A, A, DEAD]
    assert rows[0, 1, 63] == rows[0, 1, 64] == A and rows[0, 2, 62:66].tolist() == [DEAD, A, A, DEAD]  # and lanes 63 | 64
    assert wc.WIDTHS == (64, 65, 127, 128, 129, 255, 256, 257, 321)
    for W in wc.WIDTHS:
        seq = wc.lane_sequence(W, 8, turn=W)
        assert seq.shape == (2, 8 * wc.GROUP_LANES + W) and np.array_equal(seq[1], seq[0][::-1]) and wc.lane_sequence(W, 0).shape == (2, W)
    # the voxel stage's tile and workgroup edges
    keys = wc.voxel_straddle_keys()
    assert keys.shape == (2, 1, 4166) and (keys[0, 0, 1010:1040] == A).all() and (keys[0, 0, 4080:4110] == A).all()
    runs = wc.expected_runs(keys[0], 4166)
    assert (1023 // 64, 1010 % 64, 14, A) in runs and (1024 // 64, 0, 16, A) in runs and (4095 // 64, 4080 % 64, 16, A) in runs and (4096 // 64, 0, 14, A) in runs


def test_expected_runs_on_hand_written_layouts():
    # the straddle over two wavefronts: the key at lane 63 and at the next lane 0 is one key and two runs
    assert wc.expected_runs(wc.layout(("straddle_lo", "straddle_hi")), 128) == [(0, 0, 40, B), (0, 40, 24, A), (1, 0, 24, A), (1, 24, 40, B)]
    assert wc.expected_runs(wc.PATTERNS["hole"], 64) == [(0, 0, 20, A), (0, 21, 20, A), (0, 43, 21, A)]
    assert wc.expected_runs(wc.PATTERNS["lone_63"], 64) == [(0, 63, 1, A)]
    # two rows of 70 lanes: each row starts a new sequence of segments, the last segment of a row is short
    two_rows = [A] * 70 + [B] * 3 + [DEAD] + [B] * 60 + [C] * 6
    assert wc.expected_runs(two_rows, 70) == [(0, 0, 64, A), (1, 0, 6, A), (2, 0, 3, B), (2, 4, 60, B), (3, 0, 6, C)]
    assert wc.run_slices(two_rows, 70) == [(0, 64), (64, 70), (70, 73), (74, 134), (134, 140)]
    # the same lanes as ONE sequence (the voxel stage's visited pixels): a run continues from a row into the next
    assert wc.expected_runs(two_rows, 140) == [(0, 0, 64, A), (1, 0, 6, A), (1, 6, 3, B), (1, 10, 54, B), (2, 0, 6, B), (2, 6, 6, C)]
    assert wc.expected_runs([DEAD] * 64, 64) == [] and wc.expected_runs([], 64) == []
    for W in wc.WIDTHS:  # the run lengths add up to the live lanes, and no run crosses a segment
        keys = wc.row_keys(W)
        runs = wc.expected_runs(keys, W)
        assert sum(n for _, _, n, _ in runs) == int((keys >= 0).sum()) and all(lane + n <= 64 for _, lane, n, _ in runs)
        assert [b - a for a, b in wc.run_slices(keys, W)] == [n for _, _, n, _ in runs]
        assert all((keys.reshape(-1)[a:b] == k).all() for (a, b), (_, _, _, k) in zip(wc.run_slices(keys, W), runs))
        seq = wc.lane_sequence(W, 8, turn=W)
        assert sum(n for _, _, n, _ in wc.expected_runs(seq, seq.shape[1])) == int((seq >= 0).sum())


def _tv_points(sv, keys, kind, Q=wc.TV_Q):
    """The maps of a layout for disparity=kind and their points [B, H * W, 3], NaN for a pixel that is no candidate."""
    d = wc.top_view_map(keys, kind)
    return d, wc.disparity_points(sv, d, Q, kind).reshape(len(d), -1, 3)


@pytest.mark.parametrize("W", wc.WIDTHS)
def test_every_stage_realises_the_layouts(sv, W):
    """The keys recomputed from the maps with the definitions' arithmetic are the layout's, for each stage's way of placing a key."""
    keys = wc.row_keys(W)
    grid = {k: wc.TV_GRID[k] for k in ("x_range", "y_range", "z_range", "scale")}
    for kind in ("d1", "dmap"):
        _, pts = _tv_points(sv, keys, kind)
        assert np.array_equal(wc.top_view_keys(sv, pts, **grid).reshape(keys.shape), np.where(keys >= 0, keys * wc.TV_COLS + wc.TV_COL, DEAD)), kind
    _, pts = _tv_points(sv, keys, "d1", wc.TV_Q_COLUMNS)
    cells = wc.top_view_keys(sv, pts, **dict(grid, y_range=wc.TV_GRID_COLUMNS["y_range"])).reshape(keys.shape)
    assert np.array_equal(cells, wc.column_cells(keys)) and (W < 129 or len(np.unique(cells[cells >= 0] % 13)) >= 4)
    for full in (8, 0):
        seq = wc.lane_sequence(W, full, turn=W)
        assert np.array_equal(wc.top_view_keys(sv, wc.top_view_points(seq), **grid), np.where(seq >= 0, seq * wc.TV_COLS + wc.TV_COL, DEAD))
        d = wc.voxel_map(seq)
        for b in range(2):
            assert np.array_equal(wc.voxel_keys(sv, d[b][None], wc.VOXEL_Q, **wc.VOXEL_GRID), wc.voxel_key_of(seq[b]))
    for labels in wc.OCC_LABELS:
        d, lab = wc.occupancy_case(keys, labels)
        pts = wc.disparity_points(sv, d, wc.OCC_Q_SLOPE, "d1", lab)
        assert np.array_equal(wc.top_view_keys(sv, pts, **grid), np.where(keys >= 0, keys * wc.TV_COLS + wc.TV_COL, DEAD)), labels
        assert set(lab[keys >= 0].tolist()) == {"ground": {1}, "obstacle": {2}, "mix": {1, 2}}[labels]
        dead = keys < 0
        assert set(lab[dead].tolist()) == {0, 1, 2, 3} and ((d[dead] > 0) == ((lab[dead] == 0) | (lab[dead] == 3))).all()
        # the height step falls by one per column: 960 - x, so a run's largest is at its head
        h = np.trunc((pts[..., 2] + 1.0) * 512.0)
        assert np.array_equal(h[0][keys[0] >= 0], np.broadcast_to(960.0 - np.arange(W), keys[0].shape)[keys[0] >= 0])
    d, lab = wc.occupancy_blocks(W)
    pts = wc.disparity_points(sv, d, wc.OCC_Q_BLOCKS, "d1", lab)
    cells = wc.top_view_keys(sv, pts, **grid)
    assert np.array_equal(cells, wc.block_cells(d, lab)) and np.array_equal(np.trunc((pts[..., 2] + 1.0) * 512.0)[cells >= 0], d[cells >= 0])
    where = {"min": set(), "max": set()}  # of each run's smallest and largest height: at the head, the tail, the interior
    for a, b in wc.run_slices(cells, W):
        h = d.reshape(-1)[a:b]
        if b - a >= 3:
            for name, at in (("min", int(h.argmin())), ("max", int(h.argmax()))):
                where[name].add("head" if at == 0 else "tail" if at == b - a - 1 else "interior")
    assert where["min"] == where["max"] == {"head", "tail", "interior"}
    gd = wc.ground_map(keys)
    plain = (keys >= 0) & (keys != wc.TOP)
    assert np.array_equal(wc.ground_keys(sv, gd), keys) and np.array_equal(gd[plain], (keys[plain] / 4.0).astype(np.float32))
    top = gd[keys == wc.TOP]
    assert W < 256 or (np.isinf(top).any() and (top == np.float32(1e6)).any() and (top == np.float32(17.9)).any() and (top == np.float32(wc.TOP / 4)).any())


def test_the_voxel_maps_are_what_the_issue_asks_for(sv):
    """The check the issue records: a 2 x 70 map of 8 - 2^-17 with five pixels at 3.5; then the run that wraps from one image row into
    the next, on the image and on the visited lattice; the tile edges; the offsets at their largest."""
    d = np.full((2, 70), 8.0 - 2.0 ** -17, np.float32)
    d[1, :5] = 3.5
    xyz, _, cell, n, first, count = sv.voxel_cloud(d, wc.VOXEL_Q, 1.0, (0, 0, 0), (64, 64, 64), dtype="f64")
    assert count == 2 and cell.tolist() == [[7, 7, 7], [3, 3, 3]] and n.tolist() == [135, 5] and first.tolist() == [0, 70] and abs(xyz[0, 0] - 7.99999237) < 1e-8
    for step in (1, 2, 3):  # 4 x 40 visited pixels of one key: the first wavefront's run covers visited pixels 0 .. 63, row 0 and 24 of row 1
        d = np.full((4 * step, 40 * step), np.float32(B + 0.5))
        d[::step, ::step] = A + 0.5  # the lattice holds A, every pixel beside it B
        keys = wc.voxel_keys(sv, d, wc.VOXEL_Q, step=step, **wc.VOXEL_GRID)
        assert keys.tolist() == [int(wc.voxel_key_of(A))] * 160 and [r[:3] for r in wc.expected_runs(keys, 160)] == [(0, 0, 64), (1, 0, 64), (2, 0, 32)]
    keys = wc.voxel_straddle_keys()
    d = wc.voxel_map(keys)
    for b in range(2):
        assert np.array_equal(wc.voxel_keys(sv, d[b], wc.VOXEL_Q, **wc.VOXEL_GRID), wc.voxel_key_of(keys[b, 0]))
    full = wc.voxel_map(np.array(wc.PATTERNS["one_run"] + wc.PATTERNS["all_distinct"][:60])[None], wc.FULL_OFFSET)
    xyz, _, cell, n, first, count = sv.voxel_cloud(full, wc.VOXEL_Q, dtype="f64", **wc.VOXEL_GRID)
    assert count == 61 and n[0] == 64 and cell[0].tolist() == [A] * 3 and (xyz[0] == A + (64 * 65535 + 32) / (65536.0 * 64)).all()


def test_the_keep_patterns_are_what_the_issue_asks_for(sv):
    pats = wc.keep_patterns()
    assert {k: int(v.sum()) for k, v in pats.items()} == {"lane_0": 4, "lane_63": 4, "lanes_31_32": 8, "pixels_0_2": 128, "all": 256}
    for name, keep in pats.items():
        d = wc.keep_map(keep)
        for b, want in ((0, keep.reshape(-1)), (1, keep.reshape(-1)[::-1])):
            _, _, index = sv.compact_cloud(d[b], wc.VOXEL_Q, lo=wc.VOXEL_GRID["lo"], hi=wc.VOXEL_GRID["hi"])
            assert index.tolist() == np.nonzero(want)[0].tolist(), (name, b)


# ---------------------------------------------------------------------------------------------------------------- top view

def _tv_counted(eng, combine, fn):
    """fn() under sv_debug_top_view(combine, counter) -> (fn's grid as numpy, the atomics issued)."""
    import torch
    L = eng.top_view_lib()
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    try:
        torch.cuda.synchronize()
        assert L.sv_debug_top_view(combine, counter.data_ptr()) == 0
        out = fn().cpu().numpy()
        torch.cuda.synchronize()
    finally:
        L.sv_debug_top_view(1, None)
    return out, int(counter.item())


def _tv_check(sv, pts, cells, width, grid, run, what):
    """Both modes, the combine on and off: the grids equal the definition's on pts [B, N, 3], the atomics issued are the model's runs /
    the in-range points."""
    runs = wc.expected_runs(cells, width)
    for mode in ("reference", "count"):
        want = np.stack([sv.points_2_top_view(p, mode=mode, **grid) for p in pts])
        for combine in (1, 0):
            got, issued = run(mode, combine)
            assert _bits(got, want), (what, mode, combine, np.argwhere(got != want)[:4].tolist())
            assert issued == (len(runs) if combine else int((np.asarray(cells) >= 0).sum())), (what, mode, combine, issued, len(runs))


@pytest.mark.gpu
@pytest.mark.parametrize("W", wc.WIDTHS)
def test_top_view_runs_lane_by_lane(sv, eng, W):
    """Rows of nine layouts cut at W, both disparity forms, then the cell column taken from the pixel column; the points entry on the
    layouts as one long sequence and as W points."""
    keys = wc.row_keys(W)
    grid = {k: wc.TV_GRID[k] for k in ("x_range", "y_range", "z_range", "scale")}
    cases = [(kind, wc.TV_Q, grid) for kind in ("d1", "dmap")] + [("d1", wc.TV_Q_COLUMNS, dict(grid, y_range=wc.TV_GRID_COLUMNS["y_range"]))]
    for kind, Q, g in cases:
        d, pts = _tv_points(sv, keys, kind, Q)
        t = _cuda(d)
        cells = wc.top_view_keys(sv, pts, **g)
        _tv_check(sv, pts, cells, W, g, lambda mode, combine: _tv_counted(eng, combine, lambda: eng.top_view_from_disparity(t, Q, disparity=kind, mode=mode, **g)),
                  (W, kind, g["y_range"]))
    for full in (8, 0):
        pts = wc.top_view_points(wc.lane_sequence(W, full, turn=W))
        t = _cuda(pts)
        cells = wc.top_view_keys(sv, pts, **grid)
        _tv_check(sv, pts, cells, pts.shape[1], grid, lambda mode, combine: _tv_counted(eng, combine, lambda: eng.top_view(t, mode=mode, **grid)), (W, "points", full))


# ---------------------------------------------------------------------------------------------------------------- occupancy

def _occ_counted(eng, combine, fn):
    import torch
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    try:
        torch.cuda.synchronize()
        assert eng.debug_occupancy(combine, counter) == 0
        out = fn()
        torch.cuda.synchronize()
    finally:
        eng.debug_occupancy(True, None)
    return out, int(counter.item())


def _occ_check(sv, eng, d, lab, Q, grid, what):
    """The three outputs equal the definition's with the combine on and off; the counter is the model's, from the recomputed cells."""
    B, H, W = d.shape
    row, dsp = np.full((B, W), -1, np.int32), np.zeros((B, W), np.float32)  # no obstacle base: a column's line ends on its topmost ground pixel
    want = _occ_want(sv, d, lab, row, dsp, Q, **grid)
    tv = {k: grid[k] for k in ("x_range", "y_range", "z_range", "scale")}
    cells = wc.top_view_keys(sv, wc.disparity_points(sv, d, Q, "d1", lab), **tv)
    assert int(want["cells"][..., :2].sum()) == int((cells >= 0).sum()) > 0
    combined, plain = wc.occupancy_atomics(cells, lab, W)
    for combine in (True, False):
        got, issued = _occ_counted(eng, combine, lambda: _occ_gpu(eng, d, lab, row, dsp, Q, **grid))
        assert all(_bits(got[k], want[k]) for k in OCC_OUTPUTS), (what, combine, [k for k in OCC_OUTPUTS if not _bits(got[k], want[k])])
        assert issued == (combined if combine else plain), (what, combine, issued, combined, plain)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("W", wc.WIDTHS)
def test_occupancy_runs_lane_by_lane(sv, eng, W):
    """(a) the layouts as cells, the height falling along the row, under every labelling - once with z0 = -inf, where every height is
    65535 -, and (b) cells of 16 columns with the heights a permutation."""
    keys = wc.row_keys(W)
    for labels in wc.OCC_LABELS:
        d, lab = wc.occupancy_case(keys, labels)
        want = _occ_check(sv, eng, d, lab, wc.OCC_Q_SLOPE, wc.OCC_GRID, (W, labels))
        full = want["cells"][0, A, wc.TV_COL]  # the rows that hold key A alone in a whole wavefront, and more of it
        assert labels != "obstacle" or (full[1] >= 64 and full[0] == 0)
        assert (want["cells"][..., 2][want["cells"][..., 3] >= 0] < want["cells"][..., 3][want["cells"][..., 3] >= 0]).any()
    d, lab = wc.occupancy_case(keys, "mix")
    want = _occ_check(sv, eng, d, lab, wc.OCC_Q_SLOPE, dict(wc.OCC_GRID, z_range=(-np.inf, 1)), (W, "z0 = -inf"))
    assert set(want["cells"][..., 2:].reshape(-1).tolist()) == {-1, 65535}
    d, lab = wc.occupancy_blocks(W)
    _occ_check(sv, eng, d, lab, wc.OCC_Q_BLOCKS, wc.OCC_GRID, (W, "blocks"))


# ---------------------------------------------------------------------------------------------------------------- voxels

def _voxel_check(sv, eng, d, colors, what, step=1):
    """f32 and f64, the combine on and off: every frame equals the definition, and the table updates are the model's runs / the kept points."""
    keys = [wc.voxel_keys(sv, d[b], wc.VOXEL_Q, step=step, **wc.VOXEL_GRID) for b in range(len(d))]
    runs = sum(len(wc.expected_runs(k, k.size)) for k in keys)
    kept = sum(int((k >= 0).sum()) for k in keys)
    for dtype in ("f32", "f64"):
        want = sv.voxel_cloud(d, wc.VOXEL_Q, colors=colors, step=step, dtype=dtype, **wc.VOXEL_GRID)
        assert all(0 < w[5] <= wc.VOXEL_CAPACITY for w in want) and sum(int(w[3].sum()) for w in want) == kept
        res = {}
        for combine in (True, False):
            (got, counts), updates, atomics = _voxel_counters(eng, combine, lambda: _voxel_gpu(eng, d, wc.VOXEL_Q, colors=colors, step=step, dtype=dtype,
                                                                                                 capacity=wc.VOXEL_CAPACITY, **wc.VOXEL_GRID))
            assert counts.tolist() == [w[5] for w in want] and all(_voxel_same(g, w) for g, w in zip(got, want)), (what, dtype, combine, colors is not None)
            assert updates == (runs if combine else kept), (what, dtype, combine, updates, runs, kept)
            res[combine] = atomics
        assert res[True] <= res[False], (what, res)  # how many probes a claim takes depends on the schedule: no equality here


def _colors(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape + (4,), dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("W", wc.WIDTHS)
def test_voxel_runs_lane_by_lane(sv, eng, W):
    """1 x W maps: the layouts as a sequence of eight groups and a ninth cut at W, and one group alone cut at W; colours on and off."""
    for full in (8, 0):
        d = wc.voxel_map(wc.lane_sequence(W, full, turn=W))[:, None, :]
        for colors in (_colors(d.shape, W + full), None):
            _voxel_check(sv, eng, d, colors, (W, full))


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 2, 3])
def test_voxel_run_wraps_into_the_next_row(sv, eng, step):
    """4 x 40 visited pixels of one key - on the image and on the lattices of step 2 and 3 -: the first wavefront's run covers image
    row 0 and 24 pixels of row 1.  The second frame holds two keys, the change in the middle of the second visited row."""
    d = np.full((2, 4 * step, 40 * step), np.float32(B + 0.5))
    d[:, ::step, ::step] = A + 0.5
    d[1, step, 20 * step:] = C + 0.5
    for colors in (_colors(d.shape, step), None):
        _voxel_check(sv, eng, d, colors, ("wrap", step), step=step)
    assert [len(wc.expected_runs(wc.voxel_keys(sv, d[b], wc.VOXEL_Q, step=step, **wc.VOXEL_GRID), 160)) for b in range(2)] == [3, 5]


@pytest.mark.gpu
def test_voxel_runs_across_tile_and_workgroup_edges(sv, eng):
    d = wc.voxel_map(wc.voxel_straddle_keys())
    for colors in (_colors(d.shape, 4166), None):
        _voxel_check(sv, eng, d, colors, "tile edges")


@pytest.mark.gpu
@pytest.mark.parametrize("color", [(255, 255, 255, 255), (255, 0, 255, 0), (0, 255, 0, 255)])
def test_voxel_payload_extremes(sv, eng, color):
    """A whole wavefront in one voxel with every offset 65535 - 64 x 65535 per axis, the largest a run's 32-bit sums hold - and the packed
    16-bit colour sums at 64 x 255 beside 64 x 255 or beside 0, where a carry between the halves would show."""
    keys = np.array(wc.PATTERNS["one_run"] + wc.PATTERNS["all_distinct"][:60] + wc.PATTERNS["one_run"])
    d = wc.voxel_map(np.stack([keys, keys[::-1]]), wc.FULL_OFFSET)[:, None, :]
    colors = np.broadcast_to(np.array(color, np.uint8), d.shape + (4,)).copy()
    _voxel_check(sv, eng, d, colors, ("extremes", color))
    want = sv.voxel_cloud(d[0], wc.VOXEL_Q, colors=colors[0], **wc.VOXEL_GRID)
    assert want[3][0] == 128 and want[1][0].tolist() == list(color)


# ---------------------------------------------------------------------------------------------------------------- ground

@pytest.mark.gpu
@pytest.mark.parametrize("W", wc.WIDTHS)
def test_ground_histogram_runs_lane_by_lane(sv, eng, W, monkeypatch):
    """Nine rows - a strip of eight and one row of the next workgroup -, with the aggregation and without it (SV_GROUND_HIST=plain): both
    give the definition's bits on every output, and vdisp is the histogram of the recomputed keys."""
    keys = wc.row_keys(W)
    d = wc.ground_map(keys)
    model = wc.ground_keys(sv, d)
    want = [sv.ground(d[b], n_bins=wc.GROUND_BINS) for b in range(2)]
    got = {}
    for hist in ("default", "plain"):
        if hist == "plain":
            monkeypatch.setenv("SV_GROUND_HIST", "plain")
        else:
            monkeypatch.delenv("SV_GROUND_HIST", raising=False)
        got[hist] = _ground_gpu(eng, d, n_bins=wc.GROUND_BINS)
        for b in range(2):
            assert all(_bits(got[hist][k][b], want[b][k]) for k in GROUND_OUTPUTS), (W, hist, b, [k for k in GROUND_OUTPUTS if not _bits(got[hist][k][b], want[b][k])])
            for v in range(9):
                row = model[b, v]
                assert np.array_equal(got[hist]["vdisp"][b, v], np.bincount(row[row >= 0], minlength=wc.GROUND_BINS).astype(np.uint32)), (W, hist, b, v)
        assert _bits(got[hist]["vdisp"], sv.v_disparity(d, wc.GROUND_BINS))
    assert all(_bits(got["default"][k], got["plain"][k]) for k in GROUND_OUTPUTS)
    assert W < 256 or int(got["default"]["vdisp"][0, :, wc.TOP].sum()) == int((keys[0] == wc.TOP).sum()) > 0  # +inf and the bins past the last one merged with it


# ---------------------------------------------------------------------------------------------------------------- compact cloud

@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(wc.keep_patterns()))
def test_compact_cloud_ranks_from_four_ballots(sv, eng, name):
    """One wavefront of quads - 256 visited pixels - keeping what the pattern says: the rows are the definition's, in ascending pixel index."""
    keep = wc.keep_patterns()[name]
    d = wc.keep_map(keep)
    colors = _colors(d.shape, 5)
    for dtype in ("f32", "f64"):
        got, counts = _cloud_gpu(eng, d, wc.VOXEL_Q, colors, lo=wc.VOXEL_GRID["lo"], hi=wc.VOXEL_GRID["hi"], dtype=dtype)
        want = sv.compact_cloud(d, wc.VOXEL_Q, lo=wc.VOXEL_GRID["lo"], hi=wc.VOXEL_GRID["hi"], dtype=dtype, colors=colors)
        assert counts.tolist() == [int(keep.sum())] * 2
        for b in range(2):
            (gx, gc, gi), (wx, wcol, wi) = got[b], want[b]
            assert (np.diff(gi) > 0).all() and _bits(gi, wi) and _bits(gx, wx) and _bits(gc, wcol), (name, dtype, b)
