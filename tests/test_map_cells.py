"""One map, three readers: the match, the path check and the view place a world point in the same cell of the flat world map, and the
view and the frontier cells decide a cell's state alike - the rules of csrc/occupancy_map_cells.h on the device, held against their numpy
statements in stereo_vision.sv (occupancy_cells_of, occupancy_map_state).  The device counterpart of test_clearance.py's
test_cell_rule_is_the_match_s."""
import numpy as np
import pytest

from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_map_match import SMALL_MAPS, _bits

NAN, INF = float("nan"), float("inf")
ROWS, COLS = 5, 7
FRAME = dict(x_range=(0, 1), y_range=(0, 1), scale=1)  # 2 x 2 cells; cell (1, 1) stands for the vehicle point (0, 0)
FAR_D2 = 65535
VIEW_INVALID = 5


def _words(sv):
    """5 x 7 cells in negative x and y at scale 4: gx in -42 .. -38, gy in -12 .. -6."""
    return sv.occupancy_map_words(dict(dict(rows=ROWS, cols=COLS, scale=4, l_occ=85, l_free=40, l_min=-200, l_max=350), **SMALL_MAPS["negative"]))


def _points(words):
    """[(name, (tx, ty, c, s))]: the vehicle point (0, 0) under these poses is the world point under test.  Quarters of a cell at scale 4
    are multiples of 1 / 16: every product with the scale is exact and none lands on a tie but where the name says so."""
    ms = float(words["scale"])
    x_lo, x_hi, y_lo, y_hi = words["top"] - ROWS, words["top"], words["left"] - COLS, words["left"]  # the borders, in cells
    xm, ym = (x_lo + 2.25) / ms, (y_lo + 3.25) / ms                                                  # well inside
    out = []
    for name, lo, hi, mid, axis in (("x", x_lo, x_hi, ym, 0), ("y", y_lo, y_hi, xm, 1)):
        for side, border, inward in (("lo", lo, 1.0), ("hi", hi, -1.0)):
            for where, q in (("in", 0.25 * inward), ("out", -0.25 * inward)):
                v = (border + q) / ms
                out.append(("%s_%s_%s" % (name, side, where), (v, mid, 1.0, 0.0) if axis == 0 else (mid, v, 1.0, 0.0)))
    for i, gx in enumerate((x_lo + 0.25, x_hi - 0.25)):
        for j, gy in enumerate((y_lo + 0.25, y_hi - 0.25)):
            out.append(("corner_%d%d_in" % (i, j), (gx / ms, gy / ms, 1.0, 0.0)))
    for i, gx in enumerate((x_lo - 0.25, x_hi + 0.25)):
        for j, gy in enumerate((y_lo - 0.25, y_hi + 0.25)):
            out.append(("corner_%d%d_out" % (i, j), (gx / ms, gy / ms, 1.0, 0.0)))
    on = (x_lo + 2) / ms  # Xw ms is an integer: the cell above the boundary takes the point
    out += [("boundary_in", (on, ym, 1.0, 0.0)), ("boundary_negated_out", (-on, -ym, 1.0, 0.0)),
            ("border_lo_exact_in", (x_lo / ms, ym, 1.0, 0.0)), ("border_hi_exact_out", (x_hi / ms, ym, 1.0, 0.0))]
    for k in range(4):
        for what, v in (("nan", NAN), ("pinf", INF), ("ninf", -INF)):
            pose = [xm, ym, 1.0, 0.0]
            pose[k] = v
            out.append(("%s_in_word_%d_out" % (what, k), tuple(pose)))
    out.append(("huge_out", (1e300, -1e300, 1.0, 0.0)))
    return out


def test_the_points_are_what_they_claim(sv):
    """On the CPU: every border has a point inside and a point outside, the name of each point says where the definition puts it, and no
    pose with a word that is not finite is inside."""
    words = _words(sv)
    pts = _points(words)
    poses = np.array([p for _, p in pts])
    with np.errstate(invalid="ignore"):
        xy = np.stack([(poses[:, 2] * 0.0 - poses[:, 3] * 0.0) + poses[:, 0], (poses[:, 3] * 0.0 + poses[:, 2] * 0.0) + poses[:, 1]], -1)
    cells = sv.occupancy_cells_of(words, xy)
    inside = cells[:, 0] >= 0
    assert ((cells[:, 1] >= 0) == inside).all()
    for (name, pose), ok in zip(pts, inside):
        assert ok == name.endswith("_in"), name
        assert ok or not name.endswith("_in")
        if not np.isfinite(pose).all():
            assert not ok, name
    for border in ("x_lo", "x_hi", "y_lo", "y_hi"):
        assert inside[[n for n, _ in pts].index(border + "_in")] and not inside[[n for n, _ in pts].index(border + "_out")]
    named = dict(zip((n for n, _ in pts), cells.tolist()))
    assert named["x_lo_in"][0] == ROWS - 1 and named["x_hi_in"][0] == 0 and named["y_lo_in"][1] == COLS - 1 and named["y_hi_in"][1] == 0
    assert [named["corner_%d%d_in" % (i, j)] for i in (0, 1) for j in (0, 1)] == [[4, 6], [4, 0], [0, 6], [0, 0]]
    assert named["boundary_in"] == [2, 3] and named["border_lo_exact_in"] == [4, 3]


@pytest.mark.gpu
def test_one_map_three_readers(sv, eng):
    """Every point through sv_map_match_device, sv_clearance_paths_device and sv_view_device on a map whose log-odds and whose field
    name their cell: each entry equals its definition bit for bit, and all three name the cell occupancy_cells_of names."""
    words = _words(sv)
    pts = _points(words)
    poses = np.array([p for _, p in pts])
    K = len(poses)
    with np.errstate(invalid="ignore"):
        xy = np.stack([(poses[:, 2] * 0.0 - poses[:, 3] * 0.0) + poses[:, 0], (poses[:, 3] * 0.0 + poses[:, 2] * 0.0) + poses[:, 1]], -1)
    cells = sv.occupancy_cells_of(words, xy)
    inside = cells[:, 0] >= 0
    index = np.where(inside, cells[:, 0] * COLS + cells[:, 1], -1)
    at = np.arange(ROWS * COLS).reshape(ROWS, COLS)
    logodds, d2, last_seen = (at + 1).astype(np.int16), (at + 1).astype(np.uint16), np.zeros((ROWS, COLS), np.int32)

    state = np.zeros((2, 2), np.uint8)
    state[1, 1] = 2
    want = sv.occupancy_match(state, poses, FRAME, words, logodds)
    res = eng.occupancy_match(_cuda(state[None]), poses, FRAME, words, _cuda(logodds))
    sums, counts = res.sums.cpu().numpy(), res.counts.cpu().numpy()
    assert _bits(sums, want["sums"]) and _bits(counts, want["counts"]) and _bits(res.best.cpu().numpy(), want["best"])
    assert _bits(counts[0, :, 0] == 1, inside) and (counts[0, :, 1] == 0).all()
    assert (np.where(inside, sums[0, :, 0] - 1, -1) == index).all()

    centres, r2 = np.zeros((1, 2)), np.zeros(1, np.int32)
    want = sv.clearance_paths(d2, words, poses[:, None, :], centres, r2, 1)
    res = eng.clearance_paths(_cuda(d2), words, poses[:, None, :], (centres, r2), 1)
    got = {k: getattr(res, k).cpu().numpy() for k in ("first_hit", "min_d2", "n_outside")}
    assert all(_bits(got[k], want[k]) for k in got)
    assert _bits(got["n_outside"] == 0, inside) and (got["n_outside"][~inside] == 1).all()
    assert (np.where(inside, got["min_d2"] - 1, -1) == index).all() and (got["min_d2"][~inside] == FAR_D2).all()

    ends = np.zeros((1, 2))
    want = sv.occupancy_view(logodds, last_seen, words, poses[None], ends, 1, 1000, -1000)
    res = eng.occupancy_view(_cuda(logodds), _cuda(last_seen), words, poses[None], ends, 1, 1000, -1000)
    got = {k: getattr(res, k).cpu().numpy() for k in ("counts", "end_cells", "status", "best", "best_score")}
    assert all(_bits(got[k], want[k]) for k in got)
    assert got["end_cells"].shape == (1, K, 1, 2) and _bits(got["end_cells"][0, :, 0].astype(np.int32), cells)
    assert _bits(got["status"][0, :, 0] == VIEW_INVALID, ~inside)


STATE_CELLS = (15, 16, 17, 33)  # the scalar path alone, exactly one wide chunk, and a wide chunk with a cut chunk behind it (twice over)
OCCUPIED, FREE = 85, -40


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 1])
def test_state_bytes(sv, eng, offset):
    """The view's state plane and the frontier cells on maps of 15, 16, 17 and 33 cells whose log-odds stand on either side of both
    thresholds and at the ends of int16, seen and never seen - from a 16-byte aligned log-odds pointer (the wide loader) and from one 2
    bytes behind it (cell by cell)."""
    import torch
    values = np.array([OCCUPIED - 1, OCCUPIED, FREE, FREE + 1, -32768, 32767], np.int16)
    try:
        assert eng.debug_view(0, 1) == 0  # the state plane alone
        for cells in STATE_CELLS:
            for rows, cols in ((1, cells), (cells, 1)) + (((3, 11),) if cells == 33 else ((3, 5),) if cells == 15 else ()):
                k = np.arange(cells)
                for shift in range(3):
                    logodds = values[(k + shift) % 6].reshape(rows, cols)
                    last_seen = np.where((k // 6 + k + shift) % 2 == 0, 0, -1).astype(np.int32).reshape(rows, cols)  # every value with both
                    big = torch.zeros(cells + 8, dtype=torch.int16, device="cuda")
                    L = big[offset:offset + cells].view(rows, cols)
                    L.copy_(_cuda(logodds))
                    assert L.data_ptr() % 16 == 2 * offset and L.is_contiguous()
                    S = _cuda(last_seen)
                    assert S.data_ptr() % 16 == 0
                    words = dict(_words(sv), rows=rows, cols=cols)
                    res = eng.occupancy_view(L, S, words, np.array([[[0.0, 0.0, 1.0, 0.0]]]), np.zeros((1, 2)), 1, OCCUPIED, FREE)
                    plane = res.workspace[:cells].cpu().numpy().reshape(rows, cols)
                    assert _bits(plane, sv.occupancy_map_state(logodds, last_seen, OCCUPIED, FREE)), (rows, cols, shift)
                    mask = eng.frontier_cells(L, S, OCCUPIED, FREE).cpu().numpy()
                    assert _bits(mask, sv.frontier_cells(logodds, last_seen, OCCUPIED, FREE)), (rows, cols, shift)
    finally:
        assert eng.debug_view(0, 3) == 0
    seen = {(int(v), s) for shift in range(3) for k in range(33) for v, s in [(values[(k + shift) % 6], ((k // 6 + k + shift) % 2 == 0))]}
    assert seen == {(int(v), s) for v in values for s in (True, False)}  # the six log-odds crossed with last_seen 0 and -1
