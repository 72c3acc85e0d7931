"""Bird's-eye views (top views): the numpy restatement of the reference's points_2_top_view (stereo_vision/sv.py) on hand-built points
and against plain numpy fancy assignment, argument checks in Python and in the C ABI (sv_top_view_*), and the HIP rasteriser - points
entry, fused disparity entry, rig.top_view and the CLI - against the restatement, bit for bit."""
import ctypes
import os

import numpy as np
import pytest

import util
from pyoracle import ElasParams
from test_legacy_entry import _gray_cv4

SV_ERR_ARG = -1
SIZE_MAX = 2 ** 64 - 1


@pytest.fixture(scope="module")
def sv():
    return util.pkg("stereo_vision.sv")


@pytest.fixture(scope="module")
def eng():
    util.pkg("build").build()
    return util.pkg("engine")


def _reproject_np(d, Q, XR=None, XT=None, quantise=True):
    """reproject()'s arithmetic in numpy: [B,H,W,3] points of the driver's dmap (quantise) or of d itself."""
    B, H, W = d.shape
    jj, ii = np.mgrid[0:H, 0:W]
    x, y = ii.astype(np.float64)[None], jj.astype(np.float64)[None]
    v = np.clip(np.rint(d * np.float32(4.0)), 0, 255).astype(np.float64) if quantise else d.astype(np.float64)
    pos = [((Q[r, 0] * x + Q[r, 1] * y) + Q[r, 2] * v) + Q[r, 3] for r in range(4)]
    with np.errstate(divide="ignore", invalid="ignore"):
        X, Y, Z = pos[0] / pos[3], pos[1] / pos[3], pos[2] / pos[3]
        if XR is not None or XT is not None:
            XR = np.eye(3) if XR is None else np.asarray(XR, np.float64)
            XT = np.zeros(3) if XT is None else np.asarray(XT, np.float64).reshape(3)
            X, Y, Z = [((XR[r, 0] * X + XR[r, 1] * Y) + XR[r, 2] * Z) + XT[r] for r in range(3)]
    return np.stack([X, Y, Z], -1)


def _d1_points(d1, Q, XR=None, XT=None):
    """Per frame: the points of the float d1's valid pixels (d > 0) in flat order - what disparity="d1" rasterises."""
    pts = _reproject_np(d1, Q, XR, XT, quantise=False)
    return [pts[b][d1[b] > 0] for b in range(d1.shape[0])]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_hand_built_points(sv):
    f = sv.points_2_top_view
    assert f(np.zeros((0, 3)), (0, 4), (-2, 3), (-1, 1), 2).shape == (9, 11)
    assert f(np.zeros((0, 3)), (-3, 4), (-2, 3), (-1, 1), 1, mode="count").dtype == np.int32
    # strict bounds and non-finite coordinates: all dropped
    edge = np.array([[0, 0, 0], [4, 0, 0], [1, 0, 1], [1, 2, 0], [1, -2, 0], [1, 0, -1], [np.nan, 0, 0], [1, np.inf, 0], [1, 0, -np.inf],
                     [-np.inf, 0, 0], [1, np.nan, 0], [1, 0, np.nan]], np.float64)
    assert not f(edge, (0, 4), (-2, 2), (-1, 1), 1, mode="count").any()
    assert not f(edge, (0, 4), (-2, 2), (-1, 1), 1).any()
    # truncation toward zero: col = trunc(2) - trunc(-1.5) = 3 (floor would give 4)
    c = f(np.array([[1.5, -1.5, 0.0]]), (0, 4), (-2, 2), (-1, 1), 1, mode="count")
    assert c[3, 3] == 1 and c.sum() == 1
    c = f(np.array([[-0.5, -0.7, 0.0], [-1.25, 1.9, 0.0]]), (-2, 2), (-2, 2), (-1, 1), 2, mode="count")
    assert c[5, 5] == 1 and c[6, 1] == 1 and c.sum() == 2  # rows 4 - trunc(-1) / 4 - trunc(-2.5); cols 4 - trunc(-1.4) / 4 - trunc(3.8)
    # value 255 at dist 0
    g = f(np.array([[0.0, 0.0, 0.0]]), (-2, 2), (-2, 2), (-1, 1), 1)
    assert g[2, 2] == 255 and (g > 0).sum() == 1
    # max_dist = 5: dist == max_dist gives 0, dist > max_dist (|x0| > x1) gives 0 (the documented deviation) - cells occupied all the same
    pts = np.array([[-3.0, -4.0, 0.0], [-2.5, -4.9, 0.0], [2.5, 3.5, 0.0]])
    g = f(pts, (-4, 3), (-5, 4), (-1, 1), 1)
    c = f(pts, (-4, 3), (-5, 4), (-1, 1), 1, mode="count")
    assert c[6, 8] == 1 and c[5, 8] == 1 and c[1, 1] == 1 and c.sum() == 3
    assert g[6, 8] == 0 and g[5, 8] == 0 and g[1, 1] == int(((5 - np.sqrt(2.5 ** 2 + 3.5 ** 2)) / 5) * 255) > 0
    assert sv.normalize_depth(np.array([6.26]), 0, 5.0)[0] == 0
    # last writer: the largest index wins, not the largest or first value
    pts = np.array([[1.9, 0.5, 0], [5.5, 0.5, 0], [1.1, 0.9, 0], [1.5, 0.9, 0], [5.2, 0.2, 0.5]], np.float64)
    g = f(pts, (0, 10), (-5, 5), (-1, 1), 1)
    c = f(pts, (0, 10), (-5, 5), (-1, 1), 1, mode="count")
    md = np.sqrt(125.0)
    val = [int(((md - np.hypot(p[0], p[1])) / md) * 255) for p in pts]
    assert val[2] > val[3] > val[0]  # the last of the cell is neither its first, its largest nor its smallest
    assert g[9, 5] == val[3] and g[5, 5] == val[4] and (g > 0).sum() == 2
    assert c[9, 5] == 3 and c[5, 5] == 2 and c.sum() == 5
    # in_range_points keeps the reference's selection semantics
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    assert np.array_equal(sv.in_range_points(pts, x, y, z, (1.5, 10), (0, 1), (-1, 1)), pts[[0, 1, 4]])


def test_plain_numpy_assignment_agrees(sv):
    """2 M seeded points, heavy collisions, dist <= max_dist: the reference's form (fancy assignment, numpy's in-order duplicates) and
    np.add.at equal the restatement."""
    rng = np.random.default_rng(17)
    n = 2_000_000
    pts = np.stack([rng.uniform(-1, 21, n), rng.uniform(-11, 11, n), rng.uniform(-1.5, 1.5, n)], -1)
    pts[::7, :2] = np.round(pts[::7, :2], 1)  # more points on shared cells and cell edges
    xr, yr, zr, s = (0, 20), (-10, 10), (-1, 1), 2
    want = sv.points_2_top_view(pts, xr, yr, zr, s)
    cnt = sv.points_2_top_view(pts, xr, yr, zr, s, mode="count")
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    m = (x > 0) & (x < 20) & (y > -10) & (y < 10) & (z > -1) & (z < 1)
    row = (-(x[m] * s).astype(np.int32)) + int(np.trunc(20 * s))
    col = (-(y[m] * s).astype(np.int32)) + int(np.trunc(10 * s))
    md = np.sqrt(20 ** 2 + 10 ** 2)
    val = (((md - np.sqrt(x[m] ** 2 + y[m] ** 2)) / md) * 255).astype(np.uint8)
    img = np.zeros((41, 41), np.uint8)
    img[row, col] = val
    assert np.array_equal(img, want)
    acc = np.zeros((41, 41), np.int64)
    np.add.at(acc, (row, col), 1)
    assert np.array_equal(acc, cnt) and cnt.sum() == m.sum() and (cnt > 1).sum() > 1000


_BAD = [((0.5, 4), (-2, 2), (-1, 1), 1), ((0, 4), (-2, 2.25), (-1, 1), 1), ((4, 4), (-2, 2), (-1, 1), 1), ((0, 4), (2, -2), (-1, 1), 1),
        ((0, 4), (-2, 2), (1, 1), 1), ((0, 4), (-2, 2), (1, -1), 1), ((0, 4), (-2, 2), (np.nan, 1), 1), ((np.nan, 4), (-2, 2), (-1, 1), 1),
        ((0, np.inf), (-2, 2), (-1, 1), 1), ((0, 4), (-2, 2), (-1, 1), 0), ((0, 4), (-2, 2), (-1, 1), -2), ((0, 4), (-2, 2), (-1, 1), 1.5),
        ((-4, 0), (-2, 0), (-1, 1), 1), ((0, 40000), (-2, 2), (-1, 1), 1), ((0, 400), (-2, 2), (-1, 1), 100)]


def test_validation(sv, eng):
    for xr, yr, zr, s in _BAD:
        with pytest.raises(ValueError):
            sv.points_2_top_view(np.zeros((1, 3)), xr, yr, zr, s)
    with pytest.raises(ValueError):
        sv.points_2_top_view(np.zeros((1, 3)), (0, 4), (-2, 2), (-1, 1), 1, mode="max")
    # max_dist == 0 only matters in reference mode
    assert sv.points_2_top_view(np.zeros((1, 3)), (-4, 0), (-2, 0), (-1, 1), 1, mode="count").shape == (5, 3)
    L = eng.top_view_lib()

    def spec(xr, yr, zr, s, mode=0, disparity=0, reserved=None):
        sp = eng.SvTopViewSpec()
        sp.x_range[:], sp.y_range[:], sp.z_range[:] = [float(v) for v in xr], [float(v) for v in yr], [float(v) for v in zr]
        sp.scale, sp.mode, sp.disparity = int(s), mode, disparity
        if reserved is not None:
            sp.reserved[reserved] = 1
        return sp

    r, c = ctypes.c_int(-7), ctypes.c_int(-7)
    for xr, yr, zr, s in _BAD:
        if s == 1.5:  # a non-integer scale cannot reach the C struct
            continue
        sp = spec(xr, yr, zr, s)
        assert L.sv_top_view_dims(ctypes.byref(sp), ctypes.byref(r), ctypes.byref(c)) == SV_ERR_ARG, (xr, yr, zr, s)
        assert L.sv_top_view_workspace_bytes(ctypes.byref(sp), 3) == SIZE_MAX
        assert r.value == -7 and c.value == -7
    good = dict(xr=(0, 40), yr=(-20, 20), zr=(-1.4, 1.0), s=10)
    for k in range(5):
        assert L.sv_top_view_dims(ctypes.byref(spec(**good, reserved=k)), ctypes.byref(r), ctypes.byref(c)) == SV_ERR_ARG
    for mode, disparity in ((2, 0), (-1, 0), (0, 2), (1, -1)):
        assert L.sv_top_view_dims(ctypes.byref(spec(**good, mode=mode, disparity=disparity)), ctypes.byref(r), ctypes.byref(c)) == SV_ERR_ARG
    assert L.sv_top_view_dims(None, ctypes.byref(r), ctypes.byref(c)) == SV_ERR_ARG
    assert L.sv_top_view_dims(ctypes.byref(spec(**good)), None, ctypes.byref(c)) == SV_ERR_ARG
    assert L.sv_top_view_dims(ctypes.byref(spec(**good)), ctypes.byref(r), ctypes.byref(c)) == 0 and (r.value, c.value) == (401, 401)
    assert L.sv_top_view_workspace_bytes(ctypes.byref(spec(**good)), 3) == 3 * 401 * 401 * 8
    assert L.sv_top_view_workspace_bytes(ctypes.byref(spec(**good)), -1) == SIZE_MAX
    assert L.sv_top_view_workspace_bytes(ctypes.byref(spec(**good, mode=1)), 3) == 0
    assert L.sv_top_view_dims(ctypes.byref(spec((-4, 0), (-2, 0), (-1, 1), 1, mode=1)), ctypes.byref(r), ctypes.byref(c)) == 0
    assert L.sv_top_view_dims(ctypes.byref(spec((0, 4), (-2, 2), (-np.inf, np.inf), 3)), ctypes.byref(r), ctypes.byref(c)) == 0 and r.value == 13
    assert eng.top_view_spec((0, 40), (-20, 20), (-1.4, 1.0), 10)[1:] == (401, 401)
    with pytest.raises(ValueError):
        eng.top_view_spec((0, 40), (-20, 20), (-1.4, 1.0), 10, disparity="depth")


# ---------------------------------------------------------------------------------------------------------------- GPU

def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_clouds(B, N, seed, lo=-6.5, hi=6.5):
    rng = np.random.default_rng(seed)
    pts = np.round(rng.uniform(lo, hi, (B, N, 3)) * 20) / 20  # a 0.05 lattice: many points per cell, many on cell edges
    flat = pts.reshape(-1, 3)
    k = rng.integers(0, flat.size, flat.size // 50)
    flat.reshape(-1)[k] = rng.choice([np.nan, np.inf, -np.inf], k.size)
    return pts


@pytest.mark.gpu
def test_points_entry_equals_restatement(sv, eng):
    import torch
    rig = util.pkg("rig").StereoRig(1242, 375)
    try:
        _, _, cloud = rig.point_clouds(util.load_png("kitti0_color_left.png"), util.load_png("kitti0_color_right.png"), pixel_format="rgb")
    finally:
        rig.close()
    cases = [(cloud, ((-10, 10), (-4, 4), (0, 30), 8), 2000)]  # camera axes of the driver's cloud
    for B, N, seed in ((1, 1001, 1), (3, 20000 - 13, 2), (17, 4097, 3)):
        cases.append((_random_clouds(B, N, seed), ((-6, 3), (-4, 5), (-3, 3), 3), 100))  # |x0| > x1: some dist > max_dist
    for pts, (xr, yr, zr, s), min_cells in cases:
        t = _cuda(pts)
        for mode in ("reference", "count"):
            got = eng.top_view(t, xr, yr, zr, s, mode=mode).cpu().numpy()
            assert got.shape[0] == pts.shape[0]
            for b in range(pts.shape[0]):
                want = sv.points_2_top_view(pts[b].reshape(-1, 3), xr, yr, zr, s, mode=mode)
                assert got[b].dtype == want.dtype and np.array_equal(got[b], want), (mode, b, pts.shape)
                assert (want > 0).sum() >= min_cells
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def kitti_d1():
    """d1 of the colour KITTI pair 0 and two offset gray goldens, from a rig (module-scoped: one engine run)."""
    rng = np.random.default_rng(5)
    ls, rs = [util.load_png("kitti0_color_left.png")], [util.load_png("kitti0_color_right.png")]
    for k in (1, 2):
        off = rng.integers(-20, 20, 3)
        ls.append(np.clip(util.load_png("kitti%d_left.png" % k).astype(np.int64)[..., None] + off, 0, 255).astype(np.uint8))
        rs.append(np.clip(util.load_png("kitti%d_right.png" % k).astype(np.int64)[..., None] + off, 0, 255).astype(np.uint8))
    rig = util.pkg("rig").StereoRig(1242, 375)
    try:
        d1 = rig.disparity(np.stack(ls), np.stack(rs), pixel_format="rgb")
        Q = rig.Q.copy()
    finally:
        rig.close()
    return d1, Q


@pytest.mark.gpu
def test_fused_equals_unfused(sv, eng, kitti_d1):
    d1, Q = kitti_d1
    C2V = sv.CAMERA_TO_VEHICLE
    XT = np.array([0.3, -0.1, 1.65])
    t = _cuda(d1)
    grids = {None: ((-10, 10), (-4, 4), (0, 30), 8), "xf": ((0, 20), (-10, 10), (0, 3), 10)}  # quarter-depth clouds
    for xf, (xr, yr, zr, s) in grids.items():
        XR_, XT_ = (C2V, XT) if xf else (None, None)
        _, cloud = eng.reproject(t, Q, XR_, XT_, want_dmap=False)
        for mode in ("reference", "count"):
            fused = eng.top_view_from_disparity(t, Q, xr, yr, zr, s, XR=XR_, XT=XT_, mode=mode).cpu().numpy()
            unfused = eng.top_view(cloud, xr, yr, zr, s, mode=mode).cpu().numpy()
            assert np.array_equal(fused, unfused), (xf, mode)
            assert min((g > 0).sum() for g in fused) > 1500, (xf, mode)
    xr, yr, zr, s = sv.CLI_TOP_VIEW["x_range"], sv.CLI_TOP_VIEW["y_range"], sv.CLI_TOP_VIEW["z_range"], sv.CLI_TOP_VIEW["scale"]
    for XR_, XT_ in ((C2V, None), (C2V, XT)):
        want = [sv.points_2_top_view(p, xr, yr, zr, s) for p in _d1_points(d1, Q, XR_, XT_)]
        wantc = [sv.points_2_top_view(p, xr, yr, zr, s, mode="count") for p in _d1_points(d1, Q, XR_, XT_)]
        got = eng.top_view_from_disparity(t, Q, xr, yr, zr, s, XR=XR_, XT=XT_, disparity="d1").cpu().numpy()
        gotc = eng.top_view_from_disparity(t, Q, xr, yr, zr, s, XR=XR_, XT=XT_, disparity="d1", mode="count").cpu().numpy()
        for b in range(d1.shape[0]):
            assert np.array_equal(got[b], want[b]) and np.array_equal(gotc[b], wantc[b]), b
            assert (want[b] > 0).sum() > 2000


# occupied cells of the oracle's grid of pair 0 below (CLI grid, "d1", camera-to-vehicle): 22 279 - the floor keeps most of it
_MIN_OCCUPIED = 20000


@pytest.mark.gpu
def test_rig_top_view_equals_oracle(sv, oracle):
    """rig.top_view on the five colour pairs of test_rig_disparity_equals_oracle == points_2_top_view of the oracle's d1, numpy and CUDA in."""
    import torch
    rng = np.random.default_rng(11)
    ls, rs = [util.load_png("kitti0_color_left.png")], [util.load_png("kitti0_color_right.png")]
    for k in (1, 2, 3, 4):
        off = rng.integers(-40, 40, 3)
        for side, dst in (("left", ls), ("right", rs)):
            g = util.load_png("kitti%d_%s.png" % (k, side)).astype(np.int64)
            dst.append(np.clip(g[..., None] + off, 0, 255).astype(np.uint8))
    L, R = np.stack(ls), np.stack(rs)
    bgr_l, bgr_r = np.ascontiguousarray(L[..., ::-1]), np.ascontiguousarray(R[..., ::-1])
    grid = dict(sv.CLI_TOP_VIEW)
    xf = (sv.CAMERA_TO_VEHICLE, None)
    rig = util.pkg("rig").StereoRig(1242, 375)
    try:
        got = rig.top_view(bgr_l, bgr_r, pixel_format="bgr", disparity="d1", transform=xf, **grid)
        got_t = rig.top_view(_cuda(bgr_l), _cuda(bgr_r), pixel_format="bgr", disparity="d1", transform=xf, **grid)
        assert isinstance(got, np.ndarray) and isinstance(got_t, torch.Tensor) and got_t.is_cuda
        got_t = got_t.cpu().numpy()
        Q = rig.Q.copy()
        with pytest.raises(ValueError):
            rig.top_view(bgr_l, bgr_r, (0, 40), (-20, 20), (-1, 1), 0)
        with pytest.raises(ValueError):
            rig.top_view(bgr_l, bgr_r, transform="sideways", **grid)
        if rig.XR is None and rig.XT is None:
            with pytest.raises(ValueError):
                rig.top_view(bgr_l, bgr_r, transform="rig", **grid)
    finally:
        rig.close()
    assert got.shape == (5, 401, 401) and got.dtype == np.uint8
    for b in range(5):
        o1, _, _ = oracle.process(ElasParams.driver(255), _gray_cv4(L[b]), _gray_cv4(R[b]))
        want = sv.points_2_top_view(_d1_points(o1[None], Q, *xf)[0], **grid)
        if b == 0:
            assert (want > 0).sum() >= _MIN_OCCUPIED
        assert np.array_equal(got[b], want) and np.array_equal(got_t[b], want), b


@pytest.mark.gpu
def test_batches_and_repeats_and_combine(sv, eng, kitti_d1):
    """Frame b of a batch == that frame alone; three runs bitwise identical; the wave combine changes no bit and issues fewer atomics."""
    import torch
    d1, Q = kitti_d1
    t = _cuda(d1)
    L = eng.top_view_lib()
    grid = dict(sv.CLI_TOP_VIEW)
    kw = dict(XR=sv.CAMERA_TO_VEHICLE, disparity="d1")
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    try:
        for mode in ("reference", "count"):
            runs = [eng.top_view_from_disparity(t, Q, mode=mode, **kw, **grid).cpu().numpy() for _ in range(3)]
            assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
            for b in range(d1.shape[0]):
                alone = eng.top_view_from_disparity(t[b:b + 1], Q, mode=mode, **kw, **grid).cpu().numpy()
                assert np.array_equal(alone[0], runs[0][b]), (mode, b)
            issued = {}
            for combine in (1, 0):
                counter.zero_()
                torch.cuda.synchronize()
                assert L.sv_debug_top_view(combine, counter.data_ptr()) == 0
                g = eng.top_view_from_disparity(t, Q, mode=mode, **kw, **grid).cpu().numpy()
                torch.cuda.synchronize()
                issued[combine] = int(counter.item())
                assert np.array_equal(g, runs[0]), (mode, combine)
            n_points = sum(len(p[(p[:, 0] > 0) & (p[:, 0] < 40) & (p[:, 1] > -20) & (p[:, 1] < 20) & (p[:, 2] > -1.4) & (p[:, 2] < 1.0)])
                           for p in _d1_points(d1, Q, sv.CAMERA_TO_VEHICLE))
            assert issued[0] == n_points and 0 < issued[1] < issued[0], (mode, issued, n_points)
    finally:
        L.sv_debug_top_view(1, None)


@pytest.mark.gpu
def test_arithmetic_edges(sv, eng):
    """One point per frame (no collisions), placed where ((max_dist - dist) / max_dist) * 255 lies within a few ulps of an integer, and
    on cell edges: every GPU value equals numpy's - a correctly rounded sqrt and no contraction."""
    md = np.sqrt(30.0 * 30.0 + 20.0 * 20.0)
    rng = np.random.default_rng(23)
    pts = []
    for k in range(1, 255):
        dk = md * (1 - k / 255.0)
        for _ in range(6):
            th = rng.uniform(-0.5, 0.5)
            X, Y = dk * np.cos(th), dk * np.sin(th)
            for ulps in (-2, -1, 0, 1, 2):
                Xp = X
                for _ in range(abs(ulps)):
                    Xp = np.nextafter(Xp, np.inf if ulps > 0 else -np.inf)
                pts.append((Xp, Y, 0.0))
    pts = np.array(pts, np.float64)
    pts = pts[(pts[:, 0] > 0) & (pts[:, 0] < 30) & (pts[:, 1] > -20) & (pts[:, 1] < 20)]
    dist = np.sqrt(pts[:, 0] * pts[:, 0] + pts[:, 1] * pts[:, 1])
    q = ((md - dist) / md) * 255
    assert (np.abs(q - np.rint(q)) < 1e-11).sum() > 500  # many sit on the truncation's edge
    edges = []
    for k in range(1, 6 * 7):  # cell edges of x (0, 6), y (-3, 3) at scale 7 (k / 7 is not a double): on, just below, just above
        e = k / 7
        for X in (np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)):
            edges.append((X, rng.uniform(-2.9, 2.9), 0.5))
            edges.append((rng.uniform(0.1, 5.9), X - 3.0, -0.5))
            edges.append((rng.uniform(0.1, 5.9), -X + 3.0, -0.5))
    for pts, (xr, yr, zr, s) in ((pts, ((0, 30), (-20, 20), (-1, 1), 1)), (np.array(edges), ((0, 6), (-3, 3), (-1, 1), 7))):
        got = eng.top_view(_cuda(pts[:, None, :]), xr, yr, zr, s).cpu().numpy()
        want = np.stack([sv.points_2_top_view(pts[b:b + 1], xr, yr, zr, s) for b in range(len(pts))])
        assert (want > 0).sum() > 0.9 * len(pts)
        bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
        assert bad.size == 0, (bad[:10], pts[bad[:10]])


@pytest.mark.gpu
def test_top_view_on_torch_current_stream(sv, eng, kitti_d1):
    """Inputs written by a torch op on a busy side stream, no explicit synchronisation: the grids are those of the inputs at rest."""
    import torch
    d1, Q = kitti_d1
    grid = dict(sv.CLI_TOP_VIEW)
    pts = _random_clouds(4, 30000, 9)
    want_d = eng.top_view_from_disparity(_cuda(d1), Q, XR=sv.CAMERA_TO_VEHICLE, disparity="d1", **grid).cpu().numpy()
    want_p = eng.top_view(_cuda(pts), (-6, 3), (-4, 5), (-3, 3), 3, mode="count").cpu().numpy()
    src_d, src_p = _cuda(d1), _cuda(pts)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):
            x = x @ x  # keeps the stream busy while the host runs ahead
        d = torch.empty_like(src_d)
        d.copy_(src_d)
        p = torch.empty_like(src_p)
        p.copy_(src_p)
        gd = eng.top_view_from_disparity(d, Q, XR=sv.CAMERA_TO_VEHICLE, disparity="d1", **grid).clone()
        gp = eng.top_view(p, (-6, 3), (-4, 5), (-3, 3), 3, mode="count").clone()
    torch.cuda.synchronize()
    del x
    assert np.array_equal(gd.cpu().numpy(), want_d) and np.array_equal(gp.cpu().numpy(), want_p)


@pytest.mark.gpu
def test_cli_top_view_writes_rig_grids(sv, tmp_path):
    from PIL import Image
    for d in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / d)
    frames = [(util.load_png("kitti0_color_left.png"), util.load_png("kitti0_color_right.png"))]
    rng = np.random.default_rng(3)
    for k in (1, 2):
        off = rng.integers(-30, 30, 3)
        frames.append(tuple(np.clip(util.load_png("kitti%d_%s.png" % (k, s)).astype(np.int64)[..., None] + off, 0, 255).astype(np.uint8) for s in ("left", "right")))
    for i, (l, r) in enumerate(frames):
        Image.fromarray(l).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(r).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with pytest.raises(SystemExit):
        sv.main(["-k", str(tmp_path / "kitti"), "--top-view", str(tmp_path / "tv")])  # needs --batch
    sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--top-view", str(tmp_path / "tv")])
    rig = util.pkg("rig").StereoRig(1242, 375)
    try:
        want = rig.top_view(np.stack([l for l, _ in frames]), np.stack([r for _, r in frames]), pixel_format="rgb", disparity="d1",
                            transform=(sv.CAMERA_TO_VEHICLE, None), **sv.CLI_TOP_VIEW)
    finally:
        rig.close()
    for i in range(len(frames)):
        got = np.asarray(Image.open(tmp_path / "tv" / ("%010d.png" % i)))
        assert got.shape == (401, 401) and (want[i] > 0).sum() > 2000 and np.array_equal(got, want[i]), i


@pytest.mark.gpu
def test_c_abi_errors_leave_the_output_alone(eng):
    import torch
    L = eng.top_view_lib()
    sp, rows, cols = eng.top_view_spec((0, 10), (-5, 5), (-1, 1), 2)
    spc, _, _ = eng.top_view_spec((0, 10), (-5, 5), (-1, 1), 2, mode="count")
    B, N = 2, 1000
    pts = _cuda(_random_clouds(B, N, 4, 0, 9))
    disp = torch.full((B, 37, 101), 20.0, device="cuda")
    Q = np.eye(4).reshape(16)
    out = torch.full((B, rows, cols), 0x5A, dtype=torch.uint8, device="cuda")
    outc = torch.full((B, rows, cols), 0x5A5A, dtype=torch.int32, device="cuda")
    need = L.sv_top_view_workspace_bytes(ctypes.byref(sp), B)
    assert need == B * rows * cols * 8
    ws = torch.zeros(need // 8, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    p, o, w, d = pts.data_ptr(), out.data_ptr(), ws.data_ptr(), disp.data_ptr()
    cases = [L.sv_top_view_points_device(p, B, N, ctypes.byref(sp), o, w, need - 1, st),
             L.sv_top_view_points_device(p, B, N, ctypes.byref(sp), o, None, need, st),
             L.sv_top_view_points_device(p, B, N, ctypes.byref(sp), o, w + 4, need, st),
             L.sv_top_view_points_device(None, B, N, ctypes.byref(sp), o, w, need, st),
             L.sv_top_view_points_device(p, B, N, None, o, w, need, st),
             L.sv_top_view_points_device(p, B, 1 << 31, ctypes.byref(sp), o, w, 1 << 40, st),
             L.sv_top_view_points_device(p, -1, N, ctypes.byref(sp), o, w, need, st),
             L.sv_top_view_disparity_device(d, B, 101, 37, None, None, None, ctypes.byref(sp), o, w, need, st),
             L.sv_top_view_disparity_device(None, B, 101, 37, Q.ctypes.data, None, None, ctypes.byref(sp), o, w, need, st),
             L.sv_top_view_disparity_device(d, B, 101, 37, Q.ctypes.data, None, None, ctypes.byref(sp), o, w, need - 8, st),
             L.sv_top_view_disparity_device(d, B, 0, 37, Q.ctypes.data, None, None, ctypes.byref(sp), o, w, need, st),
             L.sv_top_view_disparity_device(d, B, 101, 70000, Q.ctypes.data, None, None, ctypes.byref(sp), o, w, 1 << 40, st)]
    assert cases == [SV_ERR_ARG] * len(cases)
    assert L.sv_top_view_points_device(p, B, N, ctypes.byref(spc), None, None, 0, st) == SV_ERR_ARG
    assert L.sv_top_view_points_device(p, 0, N, ctypes.byref(sp), o, w, need, st) == 0
    assert L.sv_top_view_disparity_device(d, 0, 101, 37, Q.ctypes.data, None, None, ctypes.byref(sp), o, w, need, st) == 0
    assert L.sv_top_view_points_device(p, 0, N, ctypes.byref(spc), outc.data_ptr(), None, 0, st) == 0
    torch.cuda.synchronize()
    assert (out == 0x5A).all().item() and (outc == 0x5A5A).all().item() and (ws == 0).all().item()
    # and the count mode takes no workspace
    assert L.sv_top_view_points_device(p, B, N, ctypes.byref(spc), outc.data_ptr(), None, 0, st) == 0
    torch.cuda.synchronize()
    assert outc.sum().item() == int(eng.top_view(pts, (0, 10), (-5, 5), (-1, 1), 2, mode="count").sum().item())
