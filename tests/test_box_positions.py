"""Object positions per detector box (include/stereo_vision_hip.h (E)): the numpy restatement stereo_vision.sv.box_positions on a
hand-built map and against the reference's single-accumulator order, the C ABI's argument checks, and the HIP kernel - fused disparity
entry, points entry, engine and rig layers - against the restatement bit for bit and against the legacy entry within the derived bound.

Bitwise means equal int64 views of the doubles.  Where the CPU restatement is compared with the GPU, a NaN only has to be a NaN on
both sides: IEEE 754 leaves the sign and payload of a generated NaN to the implementation (x86 SSE generates the negative quiet NaN,
the GPU the positive one).  GPU results compared with GPU results are compared whole."""
import ctypes

import numpy as np
import pytest

import util
from pyoracle import ElasParams
from test_legacy_entry import _gray_cv4
from test_top_view import _cuda, _reproject_np, eng, kitti_d1, sv  # noqa: F401 (fixtures)

SV_ERR_ARG = -1
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -53
W, H = 1242, 375
SELECTS = ("all", "valid", "near")
KINDS = ("dmap", "d1")


def _same(got, want):
    """CPU vs GPU doubles: NaN where NaN, the same bits everywhere else."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan])


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _bound(P_box):
    """2 g sum|P_i| per coordinate, g = (n - 1) u / (1 - (n - 1) u): two recursive sums of the same n terms, each within g sum|P_i|
    of the exact sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4)."""
    n = P_box.shape[0] * P_box.shape[1]
    g = (n - 1) * U / (1 - (n - 1) * U)
    return 2 * g * np.abs(P_box).reshape(-1, 3).sum(axis=0)


def _random_boxes(rng, n, w=(40, 300), h=(40, 200)):
    bw, bh = rng.integers(w[0], w[1] + 1, n), rng.integers(h[0], h[1] + 1, n)
    return np.stack([rng.integers(-20, W - 20, n), rng.integers(-20, H - 20, n), bw, bh], -1).astype(np.int32)


SPECIAL = np.array([(0, 0, W, H), (100, 100, 1, 1), (5, 5, 0, 10), (5, 5, 10, -3), (2000, 50, 30, 30), (-100, -100, 50, 50), (1200, 300, 100, 100),
                    (617, 3, 1, 350), (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (100, 50, 2 ** 31 - 1, 2 ** 31 - 1)], np.int64).astype(np.int32)

# ---------------------------------------------------------------------------------------------------------------- CPU

# 6 x 5 map, powers of two so that every term and every sum is exact whatever the order; -16 and 0 are invalid pixels
HAND_D = np.array([[1, 1, 2, 2, -16, 1],
                   [1, 0.5, 2, 2, 0.5, 1],
                   [1, 0.5, -16, 4, 0.5, 1],
                   [0.25, 0.5, 2, 4, 0, 1],
                   [1, 1, 1, 1, 1, 1]], np.float32)
HAND_Q = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 8], [0, 0, 1, 0]], np.float64)  # P = (x, y, 8) / d
HAND_BOXES = {"interior": (1, 1, 3, 2),       # columns 1..3, rows 1..2; q = 2 8 8 / 2 - 16: median 8
              "left_top": (-2, -1, 4, 3),     # clamped to columns 0..1, rows 0..1; q = 4 4 / 4 2
              "right": (3, 1, 10, 2),         # clamp(13) = 5: columns 3..4, the last column is dropped; q = 8 2 / 16 2: lower median 2, not 8
              "bottom": (1, 2, 2, 10),        # clamp(12) = 4: rows 2..3, the last row is dropped; q = 2 - / 2 8
              "w0": (2, 2, 0, 2), "hneg": (2, 2, 2, -1), "outside_hi": (10, 10, 3, 3), "outside_lo": (-10, -10, 3, 3),  # no pixel
              "one_column": (3, 0, 1, 4),     # q = 8 8 16 16
              "wide": (0, 0, 5, 4)}           # 20 pixels, three invalid
# (disparity, select, band, box): ((X, Y, Z), (n_pixels, n_valid, q_med, n_selected)), worked out by hand: "dmap" P = (x, y, 8) / q,
# "d1" P = (x, y, 8) / d; e.g. interior / d1 / near: the two q = 8 pixels (2, 1), (3, 1) -> ((2 + 3) / 2 / 2, (1 + 1) / 2 / 2, (4 + 4) / 2)
HAND = {
    ("dmap", "all", 4, "interior"): ((INF, INF, INF), (6, 5, 8, 6)),
    ("dmap", "all", 4, "left_top"): ((0.1875, 0.1875, 2.5), (4, 4, 4, 4)),
    ("dmap", "all", 4, "right"): ((1.140625, 0.4375, 2.375), (4, 4, 2, 4)),
    ("dmap", "all", 4, "bottom"): ((INF, INF, INF), (4, 3, 2, 4)),
    ("dmap", "all", 4, "w0"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "all", 4, "hneg"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "all", 4, "outside_hi"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "all", 4, "outside_lo"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "all", 4, "one_column"): ((0.28125, 0.109375, 0.75), (4, 4, 8, 4)),
    ("dmap", "all", 4, "wide"): ((INF, NAN, INF), (20, 17, 4, 20)),
    ("dmap", "valid", 4, "interior"): ((0.3625, 0.375, 2.1), (6, 5, 8, 5)),
    ("dmap", "valid", 4, "left_top"): ((0.1875, 0.1875, 2.5), (4, 4, 4, 4)),
    ("dmap", "valid", 4, "right"): ((1.140625, 0.4375, 2.375), (4, 4, 2, 4)),
    ("dmap", "valid", 4, "bottom"): ((0.4166666666666667, 0.9583333333333334, 3.0), (4, 3, 2, 3)),
    ("dmap", "valid", 4, "w0"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "valid", 4, "hneg"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "valid", 4, "outside_hi"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "valid", 4, "outside_lo"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "valid", 4, "one_column"): ((0.28125, 0.109375, 0.75), (4, 4, 8, 4)),
    ("dmap", "valid", 4, "wide"): ((0.4485294117647059, 0.5404411764705882, 2.4705882352941178), (20, 17, 4, 17)),
    ("dmap", "near", 4, "interior"): ((0.3125, 0.125, 1.0), (6, 5, 8, 2)),
    ("dmap", "near", 4, "left_top"): ((0.1875, 0.1875, 2.5), (4, 4, 4, 4)),
    ("dmap", "near", 4, "right"): ((2.0, 0.75, 4.0), (4, 4, 2, 2)),
    ("dmap", "near", 4, "bottom"): ((0.5, 1.25, 4.0), (4, 3, 2, 2)),
    ("dmap", "near", 4, "w0"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "near", 4, "hneg"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "near", 4, "outside_hi"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "near", 4, "outside_lo"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "near", 4, "one_column"): ((0.375, 0.0625, 1.0), (4, 4, 8, 2)),
    ("dmap", "near", 4, "wide"): ((0.48333333333333334, 0.5916666666666667, 2.7333333333333334), (20, 17, 4, 15)),
    ("dmap", "near", 0, "interior"): ((0.3125, 0.125, 1.0), (6, 5, 8, 2)),
    ("dmap", "near", 0, "left_top"): ((0.08333333333333333, 0.08333333333333333, 2.0), (4, 4, 4, 3)),
    ("dmap", "near", 0, "right"): ((2.0, 0.75, 4.0), (4, 4, 2, 2)),
    ("dmap", "near", 0, "bottom"): ((0.5, 1.25, 4.0), (4, 3, 2, 2)),
    ("dmap", "near", 0, "w0"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "near", 0, "hneg"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "near", 0, "outside_hi"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "near", 0, "outside_lo"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("dmap", "near", 0, "one_column"): ((0.375, 0.0625, 1.0), (4, 4, 8, 2)),
    ("dmap", "near", 0, "wide"): ((0.0625, 0.1875, 2.0), (20, 17, 4, 4)),
    ("d1", "all", 4, "interior"): ((1.1875, 1.2291666666666667, 6.916666666666667), (6, 5, 8, 6)),
    ("d1", "all", 4, "left_top"): ((0.75, 0.75, 10.0), (4, 4, 4, 4)),
    ("d1", "all", 4, "right"): ((4.5625, 1.75, 9.5), (4, 4, 2, 4)),
    ("d1", "all", 4, "bottom"): ((1.21875, 2.84375, 8.875), (4, 3, 2, 4)),
    ("d1", "all", 4, "w0"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "all", 4, "hneg"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "all", 4, "outside_hi"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "all", 4, "outside_lo"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "all", 4, "one_column"): ((1.125, 0.4375, 3.0), (4, 4, 8, 4)),
    ("d1", "all", 4, "wide"): ((INF, INF, INF), (20, 17, 4, 20)),
    ("d1", "valid", 4, "interior"): ((1.45, 1.5, 8.4), (6, 5, 8, 5)),
    ("d1", "valid", 4, "left_top"): ((0.75, 0.75, 10.0), (4, 4, 4, 4)),
    ("d1", "valid", 4, "right"): ((4.5625, 1.75, 9.5), (4, 4, 2, 4)),
    ("d1", "valid", 4, "bottom"): ((1.6666666666666667, 3.8333333333333335, 12.0), (4, 3, 2, 3)),
    ("d1", "valid", 4, "w0"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "valid", 4, "hneg"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "valid", 4, "outside_hi"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "valid", 4, "outside_lo"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "valid", 4, "one_column"): ((1.125, 0.4375, 3.0), (4, 4, 8, 4)),
    ("d1", "valid", 4, "wide"): ((1.7941176470588236, 2.161764705882353, 9.882352941176471), (20, 17, 4, 17)),
    ("d1", "near", 4, "interior"): ((1.25, 0.5, 4.0), (6, 5, 8, 2)),
    ("d1", "near", 4, "left_top"): ((0.75, 0.75, 10.0), (4, 4, 4, 4)),
    ("d1", "near", 4, "right"): ((8.0, 3.0, 16.0), (4, 4, 2, 2)),
    ("d1", "near", 4, "bottom"): ((2.0, 5.0, 16.0), (4, 3, 2, 2)),
    ("d1", "near", 4, "w0"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "near", 4, "hneg"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "near", 4, "outside_hi"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "near", 4, "outside_lo"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "near", 4, "one_column"): ((1.5, 0.25, 4.0), (4, 4, 8, 2)),
    ("d1", "near", 4, "wide"): ((1.9333333333333333, 2.3666666666666667, 10.933333333333334), (20, 17, 4, 15)),
    ("d1", "near", 0, "interior"): ((1.25, 0.5, 4.0), (6, 5, 8, 2)),
    ("d1", "near", 0, "left_top"): ((0.3333333333333333, 0.3333333333333333, 8.0), (4, 4, 4, 3)),
    ("d1", "near", 0, "right"): ((8.0, 3.0, 16.0), (4, 4, 2, 2)),
    ("d1", "near", 0, "bottom"): ((2.0, 5.0, 16.0), (4, 3, 2, 2)),
    ("d1", "near", 0, "w0"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "near", 0, "hneg"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "near", 0, "outside_hi"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "near", 0, "outside_lo"): ((NAN, NAN, NAN), (0, 0, -1, 0)),
    ("d1", "near", 0, "one_column"): ((1.5, 0.25, 4.0), (4, 4, 8, 2)),
    ("d1", "near", 0, "wide"): ((0.25, 0.75, 8.0), (20, 17, 4, 4)),
}


def test_hand_built_boxes(sv):
    names = list(HAND_BOXES)
    boxes = np.array([HAND_BOXES[n] for n in names], np.int32)
    seen = set()
    for kind in KINDS:
        for select, band in (("all", 4), ("valid", 4), ("near", 4), ("near", 0)):
            pos, stat = sv.box_positions(HAND_D, boxes, Q=HAND_Q, select=select, disparity=kind, band=band)
            assert pos.shape == (len(names), 3) and pos.dtype == np.float64 and stat.shape == (len(names), 4) and stat.dtype == np.int32
            for m, name in enumerate(names):
                want_pos, want_stat = HAND[(kind, select, band, name)]
                assert np.array_equal(pos[m], np.array(want_pos), equal_nan=True), (kind, select, band, name, pos[m])
                assert tuple(stat[m]) == want_stat, (kind, select, band, name, stat[m])
                seen.update("nan" if np.isnan(v) else "inf" if np.isinf(v) else "finite" for v in want_pos)
    assert seen == {"nan", "inf", "finite"}
    # the points form: every pixel, no disparity
    cloud = _reproject_np(HAND_D[None], HAND_Q, quantise=True)[0]
    pos, stat = sv.box_positions(cloud, boxes)
    for m, name in enumerate(names):
        want_pos, want_stat = HAND[("dmap", "all", 4, name)]
        assert np.array_equal(pos[m], np.array(want_pos), equal_nan=True) and tuple(stat[m]) == (want_stat[0], -1, -1, want_stat[0]), name
    # batched form, n_boxes: rows beyond come back NaN / -1
    pos, stat = sv.box_positions(np.stack([HAND_D, HAND_D]), np.stack([boxes, boxes[::-1]]), n_boxes=[3, 99], Q=HAND_Q, select="valid", disparity="d1")
    assert pos.shape == (2, len(names), 3) and np.isnan(pos[0, 3:]).all() and (stat[0, 3:] == -1).all()
    for m, name in enumerate(names):
        want_pos, want_stat = HAND[("d1", "valid", 4, name)]
        assert np.array_equal(pos[1, len(names) - 1 - m], np.array(want_pos), equal_nan=True) and tuple(stat[1, len(names) - 1 - m]) == want_stat
        if m < 3:
            assert np.array_equal(pos[0, m], np.array(want_pos), equal_nan=True)
    for bad in (dict(select="median"), dict(disparity="depth"), dict(band=-1), dict(band=1.5)):
        with pytest.raises(ValueError):
            sv.box_positions(HAND_D, boxes, Q=HAND_Q, **bad)
    with pytest.raises(ValueError):
        sv.box_positions(cloud, boxes, select="valid")  # a cloud has no disparity
    with pytest.raises(ValueError):
        sv.box_positions(HAND_D, boxes[:, :3], Q=HAND_Q)


KITTI_Q = np.array([[1, 0, 0, -609.5593], [0, 1, 0, -172.854], [0, 0, 0, 721.5377], [0, 0, 1 / 0.5371657, 0]], np.float64)


def test_restatement_against_the_reference_order(sv):
    """The reference's loop (stereo_vision.cpp:262-277: ONE accumulator, columns outer, rows inner) in plain Python on a seeded all-valid
    KITTI-sized map: a one-column box gives the same doubles, any other box lies within the derived bound - and the two orders do
    differ."""
    rng = np.random.default_rng(41)
    d = rng.uniform(1.0, 60.0, (H, W)).astype(np.float32)
    boxes = np.concatenate([_random_boxes(rng, 100), np.stack([rng.integers(0, W - 1, 12), rng.integers(-10, 200, 12), np.ones(12, np.int64),
                                                              rng.integers(20, 300, 12)], -1).astype(np.int32)])
    pos, stat = sv.box_positions(d, boxes, Q=KITTI_Q, select="all", disparity="dmap")
    cloud = _reproject_np(d[None], KITTI_Q, quantise=True)[0]
    assert np.isfinite(cloud).all()
    differ = worst = 0
    for m, box in enumerate(boxes):
        i_lb, i_ub, j_lb, j_ub = sv.box_bounds(box, W, H)
        assert i_ub > i_lb and j_ub > j_lb
        cols = cloud[j_lb:j_ub, i_lb:i_ub].transpose(1, 0, 2).reshape(-1, 3).tolist()  # columns outer, rows inner
        X = Y = Z = 0.0
        for p in cols:
            X += p[0]
            Y += p[1]
            Z += p[2]
        n = (i_ub - i_lb) * (j_ub - j_lb)
        ref = np.array([X / n, Y / n, Z / n])
        assert stat[m, 0] == n == stat[m, 3]
        if i_ub - i_lb == 1:
            assert _bits(pos[m], ref), (m, box)
            continue
        # the bound is on the sums; the division by n scales both and rounds each once more (half an ulp of the quotient)
        bound = _bound(cloud[j_lb:j_ub, i_lb:i_ub]) / n + U * np.abs(ref) * 2
        err = np.abs(pos[m] - ref)
        assert (err <= bound).all(), (m, box, err, bound)
        worst = max(worst, float((err / bound).max()))
        differ += not _bits(pos[m], ref)
    print("worst error / bound %.4f, %d of 100 boxes differ in a bit" % (worst, differ))
    assert differ >= 1


def _spec(eng, select=2, disparity=1, band=4, reserved=None):
    sp = eng.SvBoxSpec(select, disparity, band)
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


def _bad_calls(eng, ptr):
    """(what, return code) of every refused call of the two entries; ptr(name) gives the address of a buffer."""
    L = eng.box_lib()
    good = dict(disp=ptr("disp"), batch=2, width=16, height=8, Q=ptr("Q"), XR=None, XT=None, boxes=ptr("boxes"), n_boxes=ptr("n_boxes"), max_boxes=3,
                spec=_spec(eng), pos=ptr("pos"), stat=ptr("stat"))

    def disparity(**kw):
        a = dict(good, **kw)
        sp = ctypes.byref(a["spec"]) if a["spec"] is not None else None
        return L.sv_box_positions_disparity_device(a["disp"], a["batch"], a["width"], a["height"], a["Q"], a["XR"], a["XT"], a["boxes"], a["n_boxes"],
                                                   a["max_boxes"], sp, a["pos"], a["stat"], None)

    def points(**kw):
        a = dict(dict(good, spec=_spec(eng, 0, 0, 0)), **kw)
        sp = ctypes.byref(a["spec"]) if a["spec"] is not None else None
        return L.sv_box_positions_points_device(a["disp"], a["batch"], a["width"], a["height"], a["boxes"], a["n_boxes"], a["max_boxes"], sp, a["pos"],
                                                a["stat"], None)

    out = []
    for entry, call in (("disparity", disparity), ("points", points)):
        cases = [dict(spec=None), dict(disp=None), dict(boxes=None), dict(pos=None), dict(batch=-1), dict(batch=65536), dict(max_boxes=-1),
                 dict(max_boxes=65536), dict(width=0), dict(height=0), dict(width=-5), dict(width=65536, height=32768), dict(width=46341, height=46341)]
        cases += [dict(spec=_spec(eng, 0, 0, 0, reserved=k)) for k in range(5)]
        cases += [dict(spec=_spec(eng, s, k, b)) for s, k, b in ((3, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, -1))]
        if entry == "disparity":
            cases += [dict(Q=None), dict(spec=_spec(eng, 2, 1, -2 ** 31))]
        else:
            cases += [dict(spec=_spec(eng, 1, 0, 0)), dict(spec=_spec(eng, 2, 1, 4))]  # a cloud has no disparity to select by
        for kw in cases:
            rc = call(**kw)
            text = L.sv_last_error(None)
            out.append(((entry, sorted(kw), getattr(kw.get("spec"), "select", None)), rc, text))
    return out, disparity, points


def test_validation_needs_no_device(eng):
    """Every SV_ERR_ARG case of both entries, on host buffers: the checks run before anything touches a device, so nothing is read or
    written; batch == 0 / max_boxes == 0 return SV_OK with nothing enqueued."""
    bufs = {k: np.full(4096, 0x5A, np.uint8) for k in ("disp", "boxes", "n_boxes", "pos", "stat")}
    bufs["Q"] = np.eye(4).reshape(16)
    calls, disparity, points = _bad_calls(eng, lambda name: bufs[name].ctypes.data)
    assert len(calls) == 2 * 23 + 4
    for what, rc, text in calls:
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_box_positions"), (what, rc, text)
    for call in (disparity, points):
        assert call(batch=0) == 0 and call(max_boxes=0) == 0
    assert all((bufs[k] == 0x5A).all() for k in ("disp", "boxes", "n_boxes", "pos", "stat"))
    for bad in (dict(select="median"), dict(disparity="depth"), dict(band=-1), dict(band=2 ** 31), dict(band=0.5)):
        with pytest.raises(ValueError):
            eng.box_spec(**bad)
    sp = eng.box_spec()
    assert (sp.select, sp.disparity, sp.band, list(sp.reserved)) == (2, 1, 4, [0] * 5) and ctypes.sizeof(sp) == 32


# ---------------------------------------------------------------------------------------------------------------- GPU

def _kitti_boxes(seed=7):
    """[3, M, 4] boxes and a different count per pair: ~40 random ones per pair, then the special ones (full frame, one pixel, empty,
    off the image, over the border, one column, 32-bit overflow of x + w)."""
    rng = np.random.default_rng(seed)
    boxes = np.stack([np.concatenate([_random_boxes(rng, 40), SPECIAL[rng.permutation(len(SPECIAL))]]) for _ in range(3)])
    return boxes, np.array([boxes.shape[1], 31, 45], np.int32)


XR_T = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
XT_T = np.array([0.3, -0.1, 1.65])


@pytest.mark.gpu
@pytest.mark.parametrize("xf", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("select", SELECTS)
def test_fused_equals_restatement(sv, eng, kitti_d1, select, kind, xf):
    d1, Q = kitti_d1
    boxes, n_boxes = _kitti_boxes()
    XR_, XT_ = (XR_T, XT_T) if xf else (None, None)
    pos, stat = eng.box_positions_from_disparity(_cuda(d1), Q, _cuda(boxes), n_boxes, XR=XR_, XT=XT_, select=select, disparity=kind, band=4)
    pos, stat = pos.cpu().numpy(), stat.cpu().numpy()
    want_pos, want_stat = sv.box_positions(d1, boxes, n_boxes, Q=Q, XR=XR_, XT=XT_, select=select, disparity=kind, band=4)
    assert np.array_equal(stat, want_stat)
    bad = np.nonzero([[not _same(pos[b, m], want_pos[b, m]) for m in range(boxes.shape[1])] for b in range(3)])
    assert bad[0].size == 0, (list(zip(*bad))[:5], pos[bad][:5], want_pos[bad][:5])
    assert np.isnan(pos[1, 31:]).all() and (stat[1, 31:] == -1).all()
    assert (want_stat[0, :, 0] == (W - 1) * (H - 1)).sum() == 1 and (want_stat[0, :, 0] == 1).sum() == 1 and (want_stat[0, :, 0] == 0).sum() >= 4
    assert (want_stat[0, :, 0] == (W - 1 - 100) * (H - 1 - 50)).sum() == 1  # x + w beyond 2^31, formed in 64 bits
    if select != "all":  # the selections give usable answers: most boxes have a finite position
        assert np.isfinite(want_pos[0, :40]).all(axis=-1).sum() >= 35


@pytest.mark.gpu
def test_fused_equals_unfused(eng, kitti_d1):
    import torch
    d1, Q = kitti_d1
    boxes, n_boxes = _kitti_boxes(8)
    t = _cuda(d1)
    for XR_, XT_ in ((None, None), (XR_T, XT_T)):
        _, cloud = eng.reproject(t, Q, XR_, XT_, want_dmap=False)
        pos_p, stat_p = eng.box_positions(cloud, boxes, n_boxes)
        pos_d, stat_d = eng.box_positions_from_disparity(t, Q, boxes, n_boxes, XR=XR_, XT=XT_, select="all", disparity="dmap")
        assert _bits(pos_p.cpu().numpy(), pos_d.cpu().numpy())
        sp, sd = stat_p.cpu().numpy(), stat_d.cpu().numpy()
        used = np.arange(boxes.shape[1])[None] < n_boxes[:, None]
        assert np.array_equal(sp[..., 0], sd[..., 0]) and np.array_equal(sp[..., 3], sd[..., 3]) and (sp[..., 1:3] == -1).all()
        assert (sd[used][:, 0] == sd[used][:, 3]).all() and (sd[used][:, 1] >= 0).all()
    one, _ = eng.box_positions(cloud[1], boxes[1], None)  # one frame: [H,W,3] and [M,4]
    assert one.shape == (1, boxes.shape[1], 3) and _bits(one[0, :31].cpu().numpy(), pos_p[1, :31].cpu().numpy())
    with pytest.raises(ValueError):
        eng.box_positions(cloud.float(), boxes)
    with pytest.raises(ValueError):
        eng.box_positions(cloud, boxes[:2])
    with pytest.raises(ValueError):
        eng.box_positions(cloud, boxes.astype(np.float32))
    torch.cuda.synchronize()


def _all_positive_windows(u8, w, h, count):
    """Up to `count` (x, y, w, h) boxes, spread over the map, whose pixels (the box definition's: x..x+w-1, y..y+h-1) are all > 0."""
    z = np.zeros((u8.shape[0] + 1, u8.shape[1] + 1), np.int64)
    z[1:, 1:] = np.cumsum(np.cumsum(u8 == 0, 0), 1)
    zeros = z[h:, w:] - z[:-h, w:] - z[h:, :-w] + z[:-h, :-w]  # zeros[y, x]: window at (x, y)
    ys, xs = np.nonzero(zeros[:u8.shape[0] - 1 - h, :u8.shape[1] - 1 - w] == 0)
    pick = np.linspace(0, len(ys) - 1, min(count, len(ys))).astype(int) if len(ys) else []
    return [(int(xs[k]), int(ys[k]), w, h) for k in pick]


@pytest.mark.gpu
def test_against_the_legacy_entry(eng):
    """generatePointCloud + object_positions (sv_legacy_box_means: the reference's single accumulator over the f64 cloud on the host)
    against the fused ALL / DMAP call on the same 8-bit disparities and the legacy entry's own Q."""
    svmod = util.pkg("stereo_vision")
    rgb_l, rgb_r = util.load_png("kitti0_color_left.png"), util.load_png("kitti0_color_right.png")
    s = svmod.stereo_vision(objectTracking=False, width=W, height=H)
    try:
        cloud = np.array(s.generatePointCloud(rgb_l[..., ::-1], rgb_r[..., ::-1])).reshape(H, W, 3)
        u8 = s.last_disparity_u8()
        s.sv.sv_legacy_Q.restype = ctypes.POINTER(ctypes.c_double)
        Q = np.ctypeslib.as_array(s.sv.sv_legacy_Q(), shape=(16,)).reshape(4, 4).copy()
        finite_boxes = _all_positive_windows(u8, 60, 40, 6) + _all_positive_windows(u8, 24, 16, 6) + _all_positive_windows(u8, 1, 30, 4)
        assert len(finite_boxes) >= 3, "no all-positive window in the disparity image of kitti0"
        rng = np.random.default_rng(13)
        boxes = np.concatenate([np.array(finite_boxes, np.int32), _random_boxes(rng, 30), SPECIAL[:2], SPECIAL[6:8]])
        legacy = s.object_positions(boxes)
    finally:
        s.close()
    disp = (u8.astype(np.float32) / np.float32(4.0))[None]
    assert np.array_equal(np.clip(np.rint(disp[0] * np.float32(4.0)), 0, 255).astype(np.uint8), u8)
    pos, stat = eng.box_positions_from_disparity(_cuda(disp), Q, boxes, select="all", disparity="dmap")
    pos, stat = pos.cpu().numpy()[0], stat.cpu().numpy()[0]
    sv_ = util.pkg("stereo_vision.sv")
    n_finite = n_not = n_one_column = 0
    for m, box in enumerate(boxes):
        i_lb, i_ub, j_lb, j_ub = sv_.box_bounds(box, W, H)
        n = (i_ub - i_lb) * (j_ub - j_lb)
        assert n > 0 and stat[m, 0] == n
        P = cloud[j_lb:j_ub, i_lb:i_ub]
        for c in range(3):
            if not np.isfinite(legacy[m, c]):
                assert np.array_equal(pos[m, c], legacy[m, c], equal_nan=True), (m, box, c, pos[m], legacy[m])
            else:
                assert np.isfinite(P[..., c]).all()
                bound = _bound(P)[c] / n + 2 * U * abs(legacy[m, c])
                assert abs(pos[m, c] - legacy[m, c]) <= bound, (m, box, c, pos[m, c], legacy[m, c], bound)
        if np.isfinite(legacy[m]).all():
            n_finite += 1
            if i_ub - i_lb == 1:
                assert _bits(pos[m], legacy[m])
                n_one_column += 1
        else:
            n_not += 1
    assert n_finite >= 3 and n_not >= 1 and n_one_column >= 1, (n_finite, n_not, n_one_column)
    assert np.isfinite(legacy[:len(finite_boxes)]).all()


@pytest.mark.gpu
def test_reproducible_whatever_the_batch_and_the_order(eng, kitti_d1):
    import torch
    d1, Q = kitti_d1
    boxes, _ = _kitti_boxes(9)
    M = boxes.shape[1]
    rng = np.random.default_rng(10)
    for select, kind in (("near", "d1"), ("all", "dmap"), ("valid", "d1")):
        kw = dict(XR=XR_T, XT=XT_T, select=select, disparity=kind, band=6)
        alone_p, alone_s = [t.cpu().numpy() for t in eng.box_positions_from_disparity(_cuda(d1[1:2]), Q, boxes[1:2], **kw)]
        for _ in range(4):
            p, s = eng.box_positions_from_disparity(_cuda(d1[1:2]), Q, boxes[1:2], **kw)
            assert _bits(p.cpu().numpy(), alone_p) and np.array_equal(s.cpu().numpy(), alone_s)
        # the same pair as number 37 of 64, between other pairs with other boxes
        big_d = d1[np.arange(64) % 3].copy()
        big_b = np.stack([_random_boxes(rng, M) for _ in range(64)])
        big_d[37], big_b[37] = d1[1], boxes[1]
        p, s = eng.box_positions_from_disparity(_cuda(big_d), Q, big_b, **kw)
        assert _bits(p[37].cpu().numpy(), alone_p[0]) and np.array_equal(s[37].cpu().numpy(), alone_s[0])
        # permuted boxes: the results permute with them
        perm = rng.permutation(M)
        p, s = eng.box_positions_from_disparity(_cuda(d1[1:2]), Q, boxes[1:2, perm], **kw)
        assert _bits(p.cpu().numpy()[0], alone_p[0, perm]) and np.array_equal(s.cpu().numpy()[0], alone_s[0, perm])
    # the C entry leaves the rows at and beyond n_boxes alone (n_boxes outside [0, max_boxes] is clamped)
    L = eng.box_lib()
    t, bx = _cuda(d1), _cuda(boxes)
    nb = torch.tensor([5, -3, M + 100], dtype=torch.int32, device="cuda")
    pos = torch.full((3, M, 3), -7.25, dtype=torch.float64, device="cuda")
    stat = torch.full((3, M, 4), 0x5A5A, dtype=torch.int32, device="cuda")
    sp = eng.box_spec("near", "d1", 6)
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    st = torch.cuda.current_stream().cuda_stream
    assert L.sv_box_positions_disparity_device(t.data_ptr(), 3, W, H, q.ctypes.data, XR_T.ctypes.data, XT_T.ctypes.data, bx.data_ptr(), nb.data_ptr(), M,
                                               ctypes.byref(sp), pos.data_ptr(), stat.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert (pos[0, 5:] == -7.25).all().item() and (stat[0, 5:] == 0x5A5A).all().item() and (pos[1] == -7.25).all().item() and (stat[1] == 0x5A5A).all().item()
    assert not (stat[0, :5] == 0x5A5A).any().item() and not (stat[2] == 0x5A5A).any().item()
    assert _bits(pos[1 + 1].cpu().numpy()[:M], eng.box_positions_from_disparity(t[2:3], Q, boxes[2:3], XR=XR_T, XT=XT_T, band=6)[0].cpu().numpy()[0])
    # stat may be NULL
    pos2 = torch.full_like(pos, -7.25)
    assert L.sv_box_positions_disparity_device(t.data_ptr(), 3, W, H, q.ctypes.data, XR_T.ctypes.data, XT_T.ctypes.data, bx.data_ptr(), nb.data_ptr(), M,
                                               ctypes.byref(sp), pos2.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert _bits(pos2.cpu().numpy(), pos.cpu().numpy())


@pytest.mark.gpu
def test_refused_calls_leave_the_outputs_alone(eng):
    """The SV_ERR_ARG cases once more with device buffers: refused, nothing enqueued, pos / stat untouched."""
    import torch
    bufs = {"disp": torch.full((2, 8, 16), 20.0, device="cuda"), "boxes": torch.zeros((2, 3, 4), dtype=torch.int32, device="cuda"),
            "n_boxes": torch.full((2,), 3, dtype=torch.int32, device="cuda"), "pos": torch.full((2, 3, 3), -7.25, dtype=torch.float64, device="cuda"),
            "stat": torch.full((2, 3, 4), 0x5A5A, dtype=torch.int32, device="cuda")}
    Q = np.eye(4).reshape(16)
    calls, disparity, points = _bad_calls(eng, lambda name: Q.ctypes.data if name == "Q" else bufs[name].data_ptr())
    assert all(rc == SV_ERR_ARG for _, rc, _ in calls)
    assert disparity(batch=0) == 0 and points(max_boxes=0) == 0
    torch.cuda.synchronize()
    assert (bufs["pos"] == -7.25).all().item() and (bufs["stat"] == 0x5A5A).all().item()


@pytest.mark.gpu
def test_rig_box_positions_equals_oracle(sv, oracle):
    """rig.box_positions on colour pairs == the restatement on the oracle's d1; numpy in -> numpy out, CUDA in -> CUDA out."""
    import torch
    rng = np.random.default_rng(11)
    ls, rs = [util.load_png("kitti0_color_left.png")], [util.load_png("kitti0_color_right.png")]
    off = rng.integers(-40, 40, 3)
    for side, dst in (("left", ls), ("right", rs)):
        dst.append(np.clip(util.load_png("kitti1_%s.png" % side).astype(np.int64)[..., None] + off, 0, 255).astype(np.uint8))
    L_, R_ = np.stack(ls), np.stack(rs)
    bgr_l, bgr_r = np.ascontiguousarray(L_[..., ::-1]), np.ascontiguousarray(R_[..., ::-1])
    boxes, _ = _kitti_boxes(12)
    boxes, n_boxes = boxes[:2], np.array([boxes.shape[1], 33], np.int32)
    rigmod, engmod = util.pkg("rig"), util.pkg("engine")
    rig = rigmod.StereoRig(W, H)
    try:
        got = rig.box_positions(bgr_l, bgr_r, boxes, n_boxes)  # the defaults: "near", "d1", band 4, camera axes
        got_t = rig.box_positions(_cuda(bgr_l), _cuda(bgr_r), _cuda(boxes), _cuda(n_boxes), transform=(XR_T, XT_T), select="valid")
        got_m = rig.box_positions(bgr_l, bgr_r, boxes, n_boxes, select="all", disparity="dmap")
        assert all(isinstance(a, np.ndarray) for a in got + got_m) and all(isinstance(a, torch.Tensor) and a.is_cuda for a in got_t)
        got_t = tuple(a.cpu().numpy() for a in got_t)
        Q = rig.Q.copy()
        for bad in (dict(select="median"), dict(disparity="depth"), dict(band=-1), dict(transform="sideways")):
            with pytest.raises(ValueError):
                rig.box_positions(bgr_l, bgr_r, boxes, n_boxes, **bad)
        if rig.XR is None and rig.XT is None:
            with pytest.raises(ValueError):
                rig.box_positions(bgr_l, bgr_r, boxes, n_boxes, transform="rig")
        else:
            rig.box_positions(bgr_l, bgr_r, boxes, n_boxes, transform="rig")
    finally:
        rig.close()
    assert got[0].shape == (2, boxes.shape[1], 3) and got[0].dtype == np.float64 and got[1].shape == (2, boxes.shape[1], 4) and got[1].dtype == np.int32
    o1 = np.stack([oracle.process(ElasParams.driver(255), _gray_cv4(L_[b]), _gray_cv4(R_[b]))[0] for b in range(2)])
    for (pos, stat), kw in ((got, dict(select="near", disparity="d1")), (got_t, dict(select="valid", disparity="d1", XR=XR_T, XT=XT_T)),
                            (got_m, dict(select="all", disparity="dmap"))):
        want_pos, want_stat = sv.box_positions(o1, boxes, n_boxes, Q=Q, band=4, **kw)
        assert np.array_equal(stat, want_stat) and _same(pos, want_pos), kw
    assert np.isfinite(got[0][0, :40]).all(axis=-1).sum() >= 35
    p = engmod.SvParams.driver(255)
    p.subsampling = 1
    half = rigmod.StereoRig(W, H, params=p)
    try:
        with pytest.raises(ValueError):
            half.box_positions(bgr_l, bgr_r, boxes, n_boxes)
    finally:
        half.close()


@pytest.mark.gpu
def test_box_positions_on_torch_current_stream(eng, kitti_d1):
    """d1 and the boxes written by torch ops on a busy side stream, no explicit synchronisation: the results are those of the inputs
    at rest."""
    import torch
    d1, Q = kitti_d1
    boxes, n_boxes = _kitti_boxes(14)
    want_p, want_s = eng.box_positions_from_disparity(_cuda(d1), Q, boxes, n_boxes, XR=XR_T)
    want_p, want_s = want_p.cpu().numpy(), want_s.cpu().numpy()
    _, cloud = eng.reproject(_cuda(d1), Q, want_dmap=False)
    want_c = eng.box_positions(cloud, boxes, n_boxes)[0].cpu().numpy()
    src_d, src_b, src_n = _cuda(d1), _cuda(boxes), _cuda(n_boxes)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):
            x = x @ x  # keeps the stream busy while the host runs ahead
        d = torch.zeros_like(src_d)
        d.copy_(src_d)
        b = torch.zeros_like(src_b)
        b.copy_(src_b)
        n = torch.zeros_like(src_n)
        n.copy_(src_n)
        c = torch.zeros_like(cloud)
        c.copy_(cloud)
        gp, gs = eng.box_positions_from_disparity(d, Q, b, n, XR=XR_T)
        gc, _ = eng.box_positions(c, b, n)
        gp, gs, gc = gp.clone(), gs.clone(), gc.clone()
    torch.cuda.synchronize()
    del x
    assert _bits(gp.cpu().numpy(), want_p) and np.array_equal(gs.cpu().numpy(), want_s) and _bits(gc.cpu().numpy(), want_c)


@pytest.mark.gpu
def test_arithmetic_edges(sv, eng):
    """One pixel per box: ties of the quantiser (d = k / 4 +- 1 / 8 rounds half to even), their neighbours, NaN, +-0, the engine's -10,
    saturation (1023.75 = 4095 quarter pixels and beyond, 63.75 for the 8-bit form), infinities; then the whole row as one box with
    band 0 and with a band wider than the range."""
    vals = []
    for k in list(range(0, 12)) + [254, 255, 256, 1020, 4094, 4095, 4096]:
        for t in (k / 4.0 - 0.125, k / 4.0, k / 4.0 + 0.125):
            f = np.float32(t)
            vals += [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
    vals += [np.nan, 0.0, -0.0, -10.0, 1e-30, 63.75, 63.875, 64.0, 1023.75, 1023.875, 1024.0, 5000.0, 1e10, -1e10, 3e38, np.inf, -np.inf]
    vals = np.array(vals, np.float32)
    n = len(vals)
    d = np.zeros((1, 2, n + 1), np.float32)
    d[0, 0, :n] = vals
    boxes = np.array([(i, 0, 1, 1) for i in range(n)] + [(0, 0, n, 1), (0, 0, n - 6, 1)], np.int32)[None]
    Q = KITTI_Q.copy()
    Q[0, 3], Q[1, 3] = -3.5, -0.25
    t = _cuda(d)
    seen_q = set()
    for kind in KINDS:
        for select, band in (("all", 4), ("valid", 4), ("near", 0), ("near", 4), ("near", 5000), ("near", 2 ** 31 - 1)):
            pos, stat = eng.box_positions_from_disparity(t, Q, boxes, select=select, disparity=kind, band=band)
            want_pos, want_stat = sv.box_positions(d, boxes, Q=Q, select=select, disparity=kind, band=band)
            assert np.array_equal(stat.cpu().numpy(), want_stat), (kind, select, band, np.nonzero((stat.cpu().numpy() != want_stat).any(-1)))
            assert _same(pos.cpu().numpy(), want_pos), (kind, select, band)
            seen_q.update((kind, int(v)) for v in want_stat[0, :n, 2])
    q, valid, _ = sv.box_quantise(np.array([0.125, 0.375, 0.625, 2.125, 2.375, 1023.75, 1e10, np.nan, -10, 0.0], np.float32), "d1")
    assert q.tolist() == [0, 2, 2, 8, 10, 4095, 4095, 0, 0, 0] and valid.tolist() == [True] * 7 + [False] * 3  # half to even; saturation
    q, valid, _ = sv.box_quantise(np.array([0.125, 0.375, 63.625, 63.75, 1e10, np.nan, -10, np.inf], np.float32), "dmap")
    assert q.tolist() == [0, 2, 254, 255, 255, 0, 0, 255] and valid.tolist() == [False, True, True, True, True, False, False, True]
    assert {("d1", 4095), ("d1", 4094), ("d1", 0), ("d1", -1), ("dmap", 255), ("dmap", 1), ("dmap", -1)} <= seen_q
