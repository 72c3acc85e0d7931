"""Group (O): the frontier cells of the world map and their connected clusters.  stereo_vision.sv.frontier_cells / frontier_clusters /
frontier_goals are the definition; engine.frontier_cells / engine.frontier_clusters and rig.OccupancyMap.frontiers / frontier_goals must
equal them in shape, dtype and bits.  The masks of frontier_cases.py are painted cell by cell and checked there against the layouts
they name."""
import ctypes
import os
import re

import numpy as np
import pytest

import frontier_cases as fc
import map_stage_cases as mc
import util
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_occupancy_map import CLI_GRID, _drive_frames, drive  # noqa: F401 (drive: the committed KITTI frames' states, a fixture)
from test_clearance import _fused_recovery_maps

SV_ERR_ARG = -1
KEYS = ("label", "clusters", "sums", "info")
DTYPES = {"label": np.int32, "clusters": np.int32, "sums": np.int64, "info": np.int32}
VEHICLE_XY = (3.25, -1.5)  # where the recovery scene's frame was taken


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _same(got, want):
    """Every array of a clusters result: shape, dtype and bits."""
    return all(_bits(np.asarray(got[k]), want[k]) and want[k].dtype == DTYPES[k] for k in KEYS)


@pytest.fixture(scope="module")
def cases(sv):
    """[(name, mask, the definition's result with min_cells 1 and capacity 1024)] - computed once; the definition's labels equal the case
    file's flood fill."""
    out = []
    for name, mask, label in fc.cluster_cases():
        want = sv.frontier_clusters(mask, 1, 1024)
        assert _bits(want["label"], label), name
        out.append((name, mask, want))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_hand_case(sv):
    logodds, last_seen, pen = fc.hand_map()
    mask = sv.frontier_cells(logodds, last_seen, fc.HAND_OCCUPIED, fc.HAND_FREE, pen)
    assert _bits(mask, np.array(fc.HAND_MASK, np.uint8))
    open_mask = np.array(fc.HAND_MASK, np.uint8)
    open_mask[fc.HAND_BLOCKED] = 1
    assert _bits(sv.frontier_cells(logodds, last_seen, fc.HAND_OCCUPIED, fc.HAND_FREE), open_mask)
    assert len(np.unique(fc.components(open_mask)[open_mask != 0])) == 2 and len(np.unique(fc.components(mask)[mask != 0])) == 3  # the blocked cell splits a frontier
    # one below the thresholds: nothing is free any more, nothing is a frontier
    assert not sv.frontier_cells(logodds, last_seen, fc.HAND_OCCUPIED, fc.HAND_FREE - 1, pen).any()
    got = sv.frontier_clusters(mask, 1, 4)
    want = {"label": np.array(fc.HAND_LABEL, np.int32), "clusters": np.array(fc.HAND_ROWS, np.int32), "sums": np.array(fc.HAND_SUMS, np.int64),
            "info": np.array(fc.HAND_INFO, np.int32)}
    assert _same(got, want)
    assert _bits(got["label"], fc.components(mask))
    assert _bits(sv.frontier_clusters(mask * 200, 1, 4)["clusters"], want["clusters"])  # any non-zero byte is a member
    words = sv.occupancy_map_params((0, 6), (0, 8), 1)
    goals = sv.frontier_goals(words, got["clusters"])
    Xw, Yw = sv.occupancy_map_centres(words)
    assert goals.dtype == np.float64 and goals.tolist() == [[Xw[0], Yw[1]], [Xw[4], Yw[1]], [Xw[4], Yw[5]]]
    assert sv.occupancy_cells_of(words, goals).tolist() == [[0, 1], [4, 1], [4, 5]]
    assert sv.frontier_goals(words, np.full((3, 8), -1, np.int32)).shape == (0, 2)
    png = sv.frontier_png(got["label"], got["clusters"])
    assert png.dtype == np.uint8 and _bits(png, np.where(got["label"] == 1, 1, np.where(got["label"] == 32, 2, np.where(got["label"] == 35, 3, 0))).astype(np.uint8))
    assert sv.frontier_png(got["label"], sv.frontier_clusters(mask, 3, 4)["clusters"]).max() == 2  # the two cells of B have no row


def test_labelling_equals_scipy_on_random_masks(sv):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    for k in range(30):
        rows, cols = (int(v) for v in rng.integers(1, 41, 2))
        density = (0.0, None, 0.1, 0.45, 1.0)[k % 5]
        if density is None:  # one cell
            mask = np.zeros((rows, cols), np.uint8)
            mask[rng.integers(rows), rng.integers(cols)] = 9
        else:
            mask = (rng.random((rows, cols)) < density).astype(np.uint8) * np.uint8(1 + k)
        label = sv.frontier_labels(mask)
        ref, n = ndimage.label(mask != 0, structure=np.ones((3, 3), int))
        assert label.dtype == np.int32 and ((label >= 0) == (mask != 0)).all()
        flat, sets = label.reshape(-1), ref.reshape(-1)
        for s in range(1, n + 1):
            members = np.flatnonzero(sets == s)
            assert (flat[members] == members.min()).all(), (k, s)  # the same partition, every label the least index of its set
        assert len(np.unique(flat[flat >= 0])) == n
        assert _bits(label, fc.components(mask))


def test_case_layouts_and_the_definition_agree(cases):
    assert len(cases) > 40 and {name.split("-")[0] for name, _, _ in cases} >= {"empty", "full", "random", "checkerboard", "serpentine", "u", "comb", "corner", "pair"}
    for name, mask, want in cases:
        info = want["info"]
        assert info[2] == (mask != 0).sum() and info[0] == info[1] == len(np.unique(want["label"][mask != 0])) and info[3] == min(info[0], 1024), name


def test_cluster_options(sv):
    """min_cells against components one below, at and one above it; capacity one above, at and one below the kept; the order of the
    rows and the fill behind them."""
    mask = np.zeros((9, 12), np.uint8)
    mask[0, 9:11] = 1             # 2 cells, label 9
    mask[2, 0:3] = 1              # 3 cells, label 24
    mask[4, 5:9] = 1              # 4 cells, label 53
    mask[6:8, 0] = 1              # 2 cells, label 72
    mask[8, 8:12] = 1             # 4 cells, label 104
    sizes = {9: 2, 24: 3, 53: 4, 72: 2, 104: 4}
    for min_cells in (1, 2, 3, 4, 5):
        kept = [lab for lab in sorted(sizes) if sizes[lab] >= min_cells]
        for capacity in sorted({1, max(1, len(kept) - 1), len(kept) or 1, len(kept) + 1}):
            got = sv.frontier_clusters(mask, min_cells, capacity)
            n = min(len(kept), capacity)
            assert got["info"].tolist() == [len(kept), 5, 15, n]
            assert got["clusters"].shape == (capacity, 8) and got["sums"].shape == (capacity, 2)
            assert got["clusters"][:n, 0].tolist() == kept[:n] and got["clusters"][:n, 1].tolist() == [sizes[lab] for lab in kept[:n]]  # ascending labels
            assert (got["clusters"][n:] == -1).all() and (got["sums"][n:] == 0).all() and (got["sums"][:n] >= 0).all()
            assert _bits(got["label"], fc.components(mask))  # the labels do not depend on the options
    over = sv.frontier_clusters(mask, 1, 3)
    assert over["info"][0] == 5 > 3 == over["info"][3] and over["clusters"][:, 0].tolist() == [9, 24, 53]
    row = sv.frontier_clusters(mask, 4, 2)["clusters"]
    assert row.tolist() == [[53, 4, 4, 7, 4, 5, 4, 8], [104, 4, 8, 10, 8, 8, 8, 11]]  # cc = (2 * 26 + 4) // 8 = 7 and (2 * 38 + 4) // 8 = 10: rounded half up


def _c_clusters_call(L, base, **kw):
    a = dict(base, **kw)
    return L.sv_frontier_clusters_device(a["mask"], a["rows"], a["cols"], a["min_cells"], a["capacity"], a["label"], a["clusters"], a["sums"], a["info"], a["ws"],
                                         a["ws_bytes"], a["stream"])


def _c_cells_call(L, base, **kw):
    a = dict(base, **kw)
    return L.sv_frontier_cells_device(a["logodds"], a["last_seen"], a["pen"], a["rows"], a["cols"], a["occupied"], a["free"], a["mask"], a["stream"])


def test_validation_needs_no_device(sv, eng):
    """Every limit is refused at both sides: ValueError in the numpy form, SV_ERR_ARG from the C entries on host buffers, which stay
    untouched - the checks run before any HIP call."""
    mask = np.zeros((4, 6), np.uint8)
    for ok in (dict(min_cells=1), dict(min_cells=8000000), dict(capacity=1), dict(capacity=65535), dict(mask=np.zeros((1, 32768), np.uint8)),
               dict(mask=np.zeros((32768, 1), np.uint8)), dict(mask=np.zeros((2000, 4000), np.uint8), capacity=1)):
        assert sv.frontier_clusters(**dict(dict(mask=mask, min_cells=1, capacity=4), **ok))["info"].tolist() == [0, 0, 0, 0]
    for bad in (dict(min_cells=0), dict(min_cells=8000001), dict(min_cells=1.5), dict(min_cells=True), dict(capacity=0), dict(capacity=65536), dict(capacity=2.5),
                dict(mask=mask.astype(np.int32)), dict(mask=mask[0]), dict(mask=np.zeros((0, 4), np.uint8)), dict(mask=np.zeros((4, 0), np.uint8)),
                dict(mask=np.zeros((1, 32769), np.uint8)), dict(mask=np.zeros((32769, 1), np.uint8)), dict(mask=np.zeros((2001, 4000), np.uint8))):
        with pytest.raises(ValueError):
            sv.frontier_clusters(**dict(dict(mask=mask, min_cells=1, capacity=4), **bad))
    L16, S32 = np.zeros((4, 6), np.int16), np.zeros((4, 6), np.int32)
    for bad in (dict(logodds=L16.astype(np.int32)), dict(logodds=L16[0]), dict(last_seen=S32[:3]), dict(last_seen=S32.astype(np.int64)), dict(pen=mask[:3]),
                dict(pen=mask.astype(np.int8)), dict(occupied=0.5), dict(free=True), dict(occupied=2 ** 31), dict(free=-2 ** 31 - 1)):
        with pytest.raises(ValueError):
            sv.frontier_cells(**dict(dict(logodds=L16, last_seen=S32, occupied=85, free=-40, pen=mask), **bad))
    with pytest.raises(ValueError):
        sv.frontier_goals(sv.occupancy_map_params((0, 6), (0, 8), 1), np.zeros((3, 7), np.int32))

    L = eng.frontier_lib()
    need = ctypes.c_size_t(0)
    # two int32 per cell, a key per row, four words per 1024 cells - each block rounded up to 16
    assert L.sv_frontier_clusters_workspace(4, 6, 4, ctypes.byref(need)) == 0 and need.value == 96 + 32 + 96 + 16
    assert L.sv_frontier_clusters_workspace(1, 1, 1, ctypes.byref(need)) == 0 and need.value == 16 * 4
    assert L.sv_frontier_clusters_workspace(2000, 4000, 65535, ctypes.byref(need)) == 0 and need.value == 2 * 32000000 + 524288 + 7813 * 16
    assert L.sv_frontier_clusters_workspace(32768, 244, 1, ctypes.byref(need)) == 0 and L.sv_frontier_clusters_workspace(1, 32768, 1, ctypes.byref(need)) == 0
    keep = need.value
    for rows, cols, capacity, out in ((0, 1, 1, need), (1, 0, 1, need), (32769, 1, 1, need), (1, 32769, 1, need), (-1, 1, 1, need), (2001, 4000, 1, need),
                                      (4, 6, 0, need), (4, 6, 65536, need), (4, 6, 4, None)):
        assert L.sv_frontier_clusters_workspace(rows, cols, capacity, None if out is None else ctypes.byref(out)) == SV_ERR_ARG and need.value == keep
        assert L.sv_last_error(None).startswith(b"sv_frontier_clusters_workspace")

    bufs = {k: np.full(512, 0x5A, np.uint8) for k in ("mask", "label", "clusters", "sums", "info", "ws", "logodds", "last_seen", "pen")}
    ptr = lambda name: bufs[name].ctypes.data + (-bufs[name].ctypes.data) % 16  # noqa: E731
    base = dict(mask=ptr("mask"), rows=4, cols=6, min_cells=1, capacity=4, label=ptr("label"), clusters=ptr("clusters"), sums=ptr("sums"), info=ptr("info"), ws=ptr("ws"),
                ws_bytes=240, stream=None)
    cases = [dict(rows=0), dict(cols=0), dict(rows=32769), dict(cols=32769), dict(rows=-1), dict(rows=2001, cols=4000, ws_bytes=2 ** 40), dict(min_cells=0),
             dict(min_cells=8000001), dict(min_cells=-1), dict(capacity=0), dict(capacity=65536), dict(capacity=-1),
             dict(mask=None), dict(label=None), dict(clusters=None), dict(sums=None), dict(info=None), dict(ws=None),
             dict(label=ptr("label") + 2), dict(clusters=ptr("clusters") + 1), dict(info=ptr("info") + 2), dict(sums=ptr("sums") + 4), dict(ws=ptr("ws") + 8),
             dict(ws_bytes=239), dict(ws_bytes=0),
             # overlaps: each output with the input and with every other output, by their first and by their last bytes
             dict(label=ptr("mask")), dict(label=ptr("mask") + 20), dict(clusters=ptr("mask") + 20), dict(sums=ptr("mask") + 16), dict(info=ptr("mask") + 20),
             dict(ws=ptr("mask") + 16), dict(mask=ptr("label") + 95), dict(clusters=ptr("label") + 92), dict(sums=ptr("clusters") + 120), dict(info=ptr("sums") + 60),
             dict(info=ptr("label") + 92), dict(ws=ptr("info")), dict(info=ptr("ws") + 236), dict(sums=ptr("ws") + 232), dict(label=ptr("clusters") + 124),
             dict(clusters=ptr("sums") + 60)]
    for kw in cases:
        rc, text = _c_clusters_call(L, base, **kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_frontier_clusters:"), (sorted(kw), rc, text)
    cbase = dict(logodds=ptr("logodds"), last_seen=ptr("last_seen"), pen=ptr("pen"), rows=4, cols=6, occupied=85, free=-40, mask=ptr("mask"), stream=None)
    cases = [dict(rows=0), dict(cols=0), dict(rows=32769), dict(cols=32769), dict(cols=-1), dict(logodds=None), dict(last_seen=None), dict(mask=None),
             dict(logodds=ptr("logodds") + 1), dict(last_seen=ptr("last_seen") + 2), dict(mask=ptr("logodds")), dict(mask=ptr("logodds") + 47), dict(mask=ptr("last_seen") + 95),
             dict(mask=ptr("pen") + 23), dict(pen=ptr("mask") + 23), dict(logodds=ptr("mask") + 22)]
    for kw in cases:
        rc, text = _c_cells_call(L, cbase, **kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_frontier_cells:"), (sorted(kw), rc, text)
    assert all((b == 0x5A).all() for b in bufs.values())
    assert eng.debug_frontier(0, None) == 0
    for bad in (-1, 2, 17):
        assert eng.debug_frontier(bad, None) == SV_ERR_ARG and L.sv_last_error(None).startswith(b"sv_debug_frontier")
    assert eng.debug_frontier(0, None) == 0


def test_header_build_and_loader_agree(eng):
    """The library exports the four entries the header declares for group (O), build.py lists the new sources and header, and the module
    docstring names the forms."""
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z_]*frontier[a-z_]*)\s*\(", src))
    assert declared == {"sv_frontier_cells_device", "sv_frontier_clusters_workspace", "sv_frontier_clusters_device", "sv_debug_frontier"}
    assert text.index("/* ---- (N)") < text.index("/* ---- (O)") < text.index("/* ---- (A)")
    L = eng.frontier_lib()
    assert all(hasattr(L, n) for n in declared)
    assert len(L.sv_frontier_cells_device.argtypes) == 9 and len(L.sv_frontier_clusters_device.argtypes) == 12 and len(L.sv_frontier_clusters_workspace.argtypes) == 4
    assert set(eng.STAGE_SIGNATURES["frontier"]) == declared
    build = util.pkg("build")
    assert "frontier_kernels.hip" in build.SOURCES and "frontier.cpp" in build.SOURCES and "frontier_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("frontier_kernels.hip", "frontier.cpp", "frontier_kernels.h"))
    mc.check_map_cells(build)  # the cell rules the map's readers share are defined once
    sv_mod = util.pkg("stereo_vision.sv")
    assert all(n in sv_mod.__doc__ for n in ("frontier_cells", "frontier_clusters", "frontier_goals")) and "(O)" in sv_mod.__doc__
    assert not re.search(r"^\s*(import|from)\s+scipy", open(sv_mod.__file__).read(), flags=re.M)  # the package does not import scipy


def _explore(world):
    """The loop of the docstrings on the recovery scene -> (the unmasked frontiers' info and first rows, the frontiers under pen, the goals,
    the routes result, its xy)."""
    world.clearance(1.0)
    world.cost_to_goal((12.0, 0.0), 0.5)  # any goal: it makes the pen
    unmasked = world.frontiers(min_cells=1, reachable=False)
    unmasked = (unmasked.info.cpu().numpy().copy(), unmasked.clusters.cpu().numpy()[:4].copy())
    every = world.frontiers(min_cells=1)
    every = (every.info.cpu().numpy().copy(), every.clusters.cpu().numpy()[:6].copy())
    found = world.frontiers(min_cells=2)
    goals = world.frontier_goals(found)
    world.cost_to_goal(goals, 0.5)
    routes, xy = world.routes(VEHICLE_XY)
    return unmasked, every, found, goals, routes, xy


def test_map_class_on_cpu_tensors(sv):
    """rig.OccupancyMap.frontiers / frontier_goals on CPU tensors run the numpy definitions: the exploration loop without a GPU."""
    import torch
    (world,) = _fused_recovery_maps(sv, ["cpu"])
    world.clearance(1.0)
    with pytest.raises(ValueError):
        world.frontiers()  # reachable, and no cost_to_goal() yet
    with pytest.raises(ValueError):
        world.frontier_goals()  # no frontiers yet
    assert world.frontiers(reachable=False).info[1] == 1
    unmasked, every, found, goals, routes, xy = _explore(world)
    assert unmasked[0].tolist() == [1, 1, 176, 1] and unmasked[1][0, 1] == 176  # one component of 176 cells
    assert every[0].tolist() == [4, 4, 154, 4] and sorted(every[1][:4, 1].tolist()) == [1, 1, 1, 151] and (every[1][4:] == -1).all()
    assert isinstance(found, util.pkg("engine").FrontierResult) and found.label.dtype == torch.int32 and found.sums.dtype == torch.int64
    assert found.info.tolist() == [1, 4, 154, 1] and found.clusters.shape == (1024, 8) and found.clusters[0, 1] == 151 and (found.clusters[1:] == -1).all()
    # the numpy forms on the map's arrays
    mask = sv.frontier_cells(world.logodds.numpy(), world.last_seen.numpy(), 85, -40, world._pen.numpy())
    want = sv.frontier_clusters(mask, 2, 1024)
    assert _same({k: getattr(found, k).numpy() for k in KEYS}, want) and (world._pen.numpy() == 255).any()
    assert goals.shape == (1, 2) and goals.dtype == np.float64 and np.array_equal(goals, sv.frontier_goals(world.words, want["clusters"]))
    rep = want["clusters"][0, 2:4].tolist()
    assert sv.occupancy_cells_of(world.words, goals).tolist() == [rep] and mask[rep[0], rep[1]] == 1
    n = int(routes.length[0])
    assert routes.status.tolist() == [0] and n >= 2 and routes.cells[0, n - 1].tolist() == rep  # the route ends on the representative
    assert np.array_equal(xy[0, n - 1], goals[0])
    assert world.frontiers(min_cells=152).info.tolist() == [0, 4, 154, 0] and world.frontier_goals().shape == (0, 2)
    assert world.frontiers(min_cells=1, capacity=2).clusters.shape == (2, 8) and world.frontier_goals().shape == (2, 2)
    assert world.frontiers(min_cells=1, occupied=85, free=-500, reachable=False).info.tolist() == [0, 0, 0, 0]  # nothing is free enough


# ---------------------------------------------------------------------------------------------------------------- GPU

def _clusters_gpu(eng, mask, min_cells=1, capacity=1024, **kw):
    res = eng.frontier_clusters(_cuda(mask), min_cells, capacity, **kw)
    return res, {k: getattr(res, k).cpu().numpy() for k in KEYS}


@pytest.fixture()
def variant(eng):
    """Sets sv_debug_frontier for a test and puts the default back."""
    import torch

    def choose(v, counters=None):
        torch.cuda.synchronize()
        assert eng.debug_frontier(v, counters) == 0
    yield choose
    torch.cuda.synchronize()
    assert eng.debug_frontier(0, None) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", (0, 1))
def test_clusters_equal_the_definition(sv, eng, cases, variant, which):
    """Every painted mask, with and without the tile phase: labels, rows, sums and info."""
    variant(which)
    wrong = []
    for name, mask, want in cases:
        _, got = _clusters_gpu(eng, mask)
        if not _same(got, want):
            wrong.append((name, [k for k in KEYS if not _bits(got[k], want[k])], got["info"].tolist(), want["info"].tolist()))
    assert not wrong, wrong
    # rows dropped by min_cells and by capacity: the ranks of the roots without a row
    for name, mask, _ in cases:
        if name.startswith("random-") or name in ("tile-corners", "both-corner-diagonals"):
            for min_cells, capacity in ((1, 3), (2, 1024), (3, 2)):
                _, got = _clusters_gpu(eng, mask, min_cells, capacity)
                assert _same(got, sv.frontier_clusters(mask, min_cells, capacity)), (name, min_cells, capacity)


@pytest.mark.gpu
def test_the_tile_phase_does_its_work(sv, eng, variant):
    import torch
    mask, n_tiles = fc.inside_tiles_mask()
    want = sv.frontier_clusters(mask, 1, 4096)
    assert want["info"][1] > 100
    counters = torch.zeros(2, dtype=torch.int64, device="cuda")
    variant(0, counters)
    _, got = _clusters_gpu(eng, mask, 1, 4096)
    assert _same(got, want) and counters.cpu().tolist() == [0, n_tiles]  # no component reaches over a seam: not one atomic on global memory
    mask[63, 5] = mask[64, 5] = 1  # one pair over a seam
    assert "h" in fc.crossings(mask)
    counters.zero_()
    _, got = _clusters_gpu(eng, mask, 1, 4096)
    first = counters.cpu().tolist()
    assert _same(got, sv.frontier_clusters(mask, 1, 4096)) and first[0] >= 1 and first[1] == n_tiles
    counters.zero_()
    variant(1, counters)
    _, got = _clusters_gpu(eng, mask, 1, 4096)
    flat = counters.cpu().tolist()
    assert _same(got, sv.frontier_clusters(mask, 1, 4096)) and flat[0] > first[0] and flat[1] == 0  # every link through global memory, no tile kernel


def _view(a, offset):
    """a on the device as a contiguous view that starts `offset` elements into its storage: 16-byte aligned with 0, not with 1."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    store = torch.zeros(a.size + 64, dtype=t.dtype, device="cuda")
    v = store[offset:offset + a.size].view(a.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (offset == 0)
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("shape", fc.CELLS_SHAPES, ids=lambda s: "%dx%d" % s)
def test_cells_equal_the_definition(sv, eng, shape):
    """Random maps with and without pen, aligned - the 16-cell chunks - and misaligned - cell by cell -, thresholds at, below and above
    the log-odds present."""
    import torch
    logodds, last_seen, pen = fc.cells_map(shape, 3 + shape[0])
    seen = 0
    for off_in, off_out in ((0, 0), (1, 0), (0, 1), (1, 1)):
        L, S, P = _view(logodds, off_in), _view(last_seen, off_in), _view(pen, off_out)
        out = _view(np.full(shape, 0x5A, np.uint8), off_out)
        for occupied, free in fc.CELLS_THRESHOLDS if (off_in, off_out) in ((0, 0), (1, 1)) else fc.CELLS_THRESHOLDS[4:5]:
            for with_pen in (True, False):
                want = sv.frontier_cells(logodds, last_seen, occupied, free, pen if with_pen else None)
                got = eng.frontier_cells(L, S, occupied, free, P if with_pen else None, out=out)
                assert got is out and _bits(got.cpu().numpy(), want), (off_in, off_out, occupied, free, with_pen)
                seen += int(want.sum())
    assert seen > 0 or shape == (1, 1)
    fresh = eng.frontier_cells(_cuda(logodds), _cuda(last_seen), 85, -40)
    assert fresh.dtype == torch.uint8 and _bits(fresh.cpu().numpy(), sv.frontier_cells(logodds, last_seen, 85, -40))


@pytest.mark.gpu
def test_mechanics(sv, eng, cases):
    """out= and the workspace reused across two different masks, a stream of its own, two calls back to back, and refusals that enqueue
    nothing."""
    import torch
    by_name = {name: (mask, want) for name, mask, want in cases}
    first, second = by_name["random-129x130"], by_name["tile-corners"]  # many rows, then few: nothing stale may stay
    res, got = _clusters_gpu(eng, first[0])
    assert _same(got, first[1]) and first[1]["info"][3] > second[1]["info"][3] == 4
    again = eng.frontier_clusters(_cuda(second[0]), out=res, workspace=res.workspace)
    assert again.label is res.label and again.clusters is res.clusters and again.workspace is res.workspace
    assert _same({k: getattr(again, k).cpu().numpy() for k in KEYS}, second[1])
    back = eng.frontier_clusters(_cuda(first[0]), out=(res.label, res.clusters, res.sums, res.info), workspace=res.workspace)
    twice = eng.frontier_clusters(_cuda(first[0]))
    assert all(torch.equal(getattr(back, k), getattr(twice, k)) for k in KEYS) and _same({k: getattr(back, k).cpu().numpy() for k in KEYS}, first[1])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        mask_t = _cuda(first[0])
        on = eng.frontier_clusters(mask_t, 2, 7)
        cells = eng.frontier_cells(_cuda(np.zeros((5, 5), np.int16)), _cuda(np.full((5, 5), -1, np.int32)), 85, 0)
    stream.synchronize()
    assert _same({k: getattr(on, k).cpu().numpy() for k in KEYS}, sv.frontier_clusters(first[0], 2, 7)) and not cells.cpu().numpy().any()
    # refused: the outputs keep their bytes
    mask_t = _cuda(second[0])
    marks = [torch.full_like(getattr(res, k), 77) for k in KEYS]
    small = torch.empty(res.workspace.numel() - 1, dtype=torch.uint8, device="cuda")
    for bad in (dict(min_cells=0), dict(capacity=0), dict(capacity=65536), dict(workspace=small), dict(out=(marks[0], marks[1], marks[2])), dict(out=(marks[0].view(-1), marks[1], marks[2], marks[3])),
                dict(out=(marks[0], marks[1], marks[2].int(), marks[3])), dict(mask=mask_t.cpu()), dict(mask=mask_t.int()), dict(mask=mask_t[:, :100])):
        with pytest.raises(ValueError):
            eng.frontier_clusters(**dict(dict(mask=mask_t, min_cells=1, capacity=1024, out=tuple(marks)), **bad))
    L = eng.frontier_lib()
    rows, cols = second[0].shape
    args = lambda **kw: _c_clusters_call(L, dict(mask=mask_t.data_ptr(), rows=rows, cols=cols, min_cells=1, capacity=1024, label=marks[0].data_ptr(), clusters=marks[1].data_ptr(),  # noqa: E731
                                                 sums=marks[2].data_ptr(), info=marks[3].data_ptr(), ws=res.workspace.data_ptr(), ws_bytes=res.workspace.numel(), stream=None), **kw)
    for kw in (dict(ws_bytes=res.workspace.numel() - 1), dict(label=marks[0].data_ptr() + 2), dict(sums=marks[1].data_ptr()), dict(min_cells=0), dict(info=mask_t.data_ptr())):
        assert args(**kw) == SV_ERR_ARG
    torch.cuda.synchronize()
    assert all((m == 77).all().item() for m in marks)
    assert args() == 0
    torch.cuda.synchronize()
    assert _same(dict(zip(KEYS, (m.cpu().numpy() for m in marks))), second[1])


@pytest.mark.gpu
def test_map_class_on_the_device(sv, eng, drive):
    """rig.OccupancyMap on the device against the class on CPU tensors: the exploration loop on the recovery scene, route included; and
    the committed drive's map against the numpy forms."""
    world, cpu = _fused_recovery_maps(sv, ["cuda", "cpu"])
    with pytest.raises(ValueError):
        world.frontiers()
    (unmasked, every, found, goals, routes, xy), (unmasked_cpu, every_cpu, found_cpu, goals_cpu, routes_cpu, xy_cpu) = _explore(world), _explore(cpu)
    assert found.label.is_cuda and found.workspace is not None
    for a, b in ((unmasked, unmasked_cpu), (every, every_cpu)):
        assert _bits(a[0], b[0]) and _bits(a[1], b[1])
    assert _same({k: getattr(found, k).cpu().numpy() for k in KEYS}, {k: getattr(found_cpu, k).numpy() for k in KEYS}) and found_cpu.info.tolist() == [1, 4, 154, 1]
    assert _bits(goals, goals_cpu) and goals.shape == (1, 2)
    assert all(_bits(getattr(routes, k).cpu().numpy(), getattr(routes_cpu, k).numpy()) for k in ("cells", "length", "status")) and np.array_equal(xy, xy_cpu, equal_nan=True)
    assert routes_cpu.status.tolist() == [0]
    again = world.frontiers(min_cells=2)
    assert again.label is found.label and again.workspace is found.workspace  # the tensors stay with the map

    _, _, _, words, fused = drive
    logodds, last_seen = fused["logodds"], fused["last_seen"]
    pen = sv.cost_cells(sv.occupancy_clearance(logodds, 10, 85), 25, radius=10)
    for p in (None, pen):
        want_mask = sv.frontier_cells(logodds, last_seen, 85, -40, p)
        mask = eng.frontier_cells(_cuda(logodds), _cuda(last_seen), 85, -40, None if p is None else _cuda(p))
        assert _bits(mask.cpu().numpy(), want_mask) and want_mask.sum() > 100
        res = eng.frontier_clusters(mask, 8, 64)
        want = sv.frontier_clusters(want_mask, 8, 64)
        assert _same({k: getattr(res, k).cpu().numpy() for k in KEYS}, want) and want["info"][3] >= 1
        assert _bits(sv.frontier_goals(words, res.clusters.cpu().numpy()), sv.frontier_goals(words, want["clusters"]))


@pytest.mark.gpu
def test_cli_prints_the_clusters_and_writes_the_labels(sv, eng, drive, tmp_path, capsys):
    from PIL import Image
    _, states, _, _, _ = drive
    n = 2
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    ls, rs = _drive_frames(n)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    xyyaw = np.array([[0.0, 0.0, 0.0], [0.9, 0.1, 0.02]])
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("".join("%r %r %r\n" % tuple(float(v) for v in row) for row in xyyaw))
    out = str(tmp_path / "map.png")
    common = ["-k", str(tmp_path / "kitti"), "--batch", "2"]
    with_map = ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt")]
    for bad in (["--frontiers", "3"], with_map + ["--frontiers", "3"], ["--occupancy-map", out, "--clearance", "1.0", "--frontiers", "3"],
                with_map + ["--clearance", "1.0", "--frontiers", "-1"], with_map + ["--clearance", "1.0", "--frontiers", "8000001"], with_map + ["--clearance", "1.0", "--frontiers", "x"]):
        with pytest.raises(SystemExit):
            sv.main(common + bad)
    assert not os.path.exists(out)
    # the definition on CPU tensors: the map of the two frames, the pen of a field towards the last pose, the clusters, the field towards them
    ranges = sv.occupancy_map_cover(xyyaw, sv.CLI_TOP_VIEW["x_range"], sv.CLI_TOP_VIEW["y_range"])
    cpu = util.pkg("rig").OccupancyMap(ranges[0], ranges[1], 10, device="cpu")
    cpu.update(states[:2], sv.occupancy_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2]), CLI_GRID)
    cpu.clearance(1.0)
    cpu.cost_to_goal(xyyaw[-1, :2], 1.0)
    found = cpu.frontiers(min_cells=3)
    lines = sv.frontier_lines(cpu.words, found.clusters.numpy(), found.info.numpy())
    print(lines[0])
    assert found.info[3] >= 1 and len(lines) == 1 + int(found.info[3]) and lines[1].startswith("frontier 0: %d cells, representative (" % int(found.clusters[0, 1]))
    field = cpu.cost_to_goal(cpu.frontier_goals(found), 1.0)
    routes, _ = cpu.routes(xyyaw[-1, :2])
    capsys.readouterr()
    sv.main(common + with_map + ["--clearance", "1.0", "--frontiers", "3"])
    printed = capsys.readouterr().out
    assert "".join(line + "\n" for line in lines) in printed
    start, length = routes.cells[0, 0].tolist(), int(routes.length[0])
    assert "route: status %d, %d cells, cost at the start %s\n" % (int(routes.status[0]), length, int(field.cost[start[0], start[1]]) if length else None) in printed
    got = np.asarray(Image.open(str(tmp_path / "map.frontiers.png")))
    want = sv.frontier_png(found.label.numpy(), found.clusters.numpy())
    assert got.dtype == np.uint8 and np.array_equal(got, want) and want.max() == min(int(found.info[3]), 255)
