"""Voxel-grid downsampled clouds (include/stereo_vision_hip.h (I)): the numpy definition stereo_vision.sv.voxel_cloud on a hand-built map
and against an independent derivation over compact_cloud's list, the C ABI's argument checks, write_ply, and the HIP kernels - C entry,
engine, rig and CLI layers - against the definition.

On the GPU everything is compared bitwise (integer views of the floats) and the counts exactly: a voxel's sums are integers, so they do
not depend on the order in which its points arrive, and the row is one fixed double expression of them."""
import ctypes
import functools
import os

import numpy as np
import pytest

import util
from test_compact_cloud import (HAND_D, HAND_Q, HAND_XR, HAND_XT, SMALL_Q, XR_G, XT_G, _bits, _colour_pairs, _random_map,  # noqa: F401
                                _read_ply)
from test_top_view import _cuda, eng, kitti_d1, sv  # noqa: F401 (fixtures)

SV_ERR_ARG = -1
SIZE_MAX = 2 ** 64 - 1
NAN, INF = float("nan"), float("inf")
W, H = 1242, 375
KITTI_Q = np.array([[1, 0, 0, -609.5593], [0, 1, 0, -172.854], [0, 0, 0, 721.5377], [0, 0, 1 / 0.5372, 0]], np.float64)
CLI_LO, CLI_HI = (0.0, -20.0, -1.4), (40.0, 20.0, 1.0)
CAM_LO, CAM_HI = (-20.0, -3.0, 0.5), (20.0, 2.0, 40.0)  # camera axes: right, down, forward
C2V = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


# ---------------------------------------------------------------------------------------------------------------- CPU

# HAND_D / HAND_Q of test_compact_cloud: P = (x, y, 8) / d ("d1"), pixel (x, y) has index 6 y + x.  Crop (-1, -1, 0) .. (11, 9, 24), size 4:
# 3 x 3 x 6 cells, t = ((X + 1) / 4, (Y + 1) / 4, Z / 4), every quotient exact.  Pixels 7, 14, 23 (Z = 64, 32, 64) are outside.
# voxel: (cell, member pixels in pixel order, S = sum of the offsets u = frac(t) * 65536), listed in ascending first member
HAND_VOXELS = [
    ((0, 0, 2), [0, 12, 13], (65536, 114688, 0)),            # t = (.25, .25, 2), (.25, .75, 2), (.5, .75, 2)
    ((0, 0, 1), [1, 8, 15, 22, 24], (163840, 163840, 0)),    # (.375, .25, 1), (.5, .375, 1), (.625, .5, 1), (.75, .625, 1), (.25, .75, 1)
    ((0, 0, 0), [3, 11, 17, 25, 27], (135168, 116736, 131072)),
    ((2, 0, 4), [4], (16384, 16384, 0)),                     # P = (8, 0, 16)
    ((1, 0, 2), [5, 10], (49152, 49152, 0)),                 # (1.5, .25, 2), (1.25, .5, 2)
    ((0, 1, 4), [18], (16384, 49152, 0)),                    # P = (0, 6, 16)
    ((0, 1, 2), [20], (49152, 0, 0)),                        # P = (2, 3, 8): Y + 1 = 4 lies exactly on the face between cells 0 and 1 -> cell 1, u = 0
    ((1, 1, 2), [21, 28], (16384, 16384, 0)),                # P = (3, 3, 8) on two faces: t = (1, 1, 2), u = 0; and (1.25, 1.25, 2)
    ((2, 2, 4), [29], (49152, 16384, 0)),                    # P = (10, 8, 16)
]
# step 2 visits pixels 0, 4, 12, 14, 24, 28 (2 is -16, 26 NaN; 14 is outside)
HAND_VOXELS_STEP2 = [((0, 0, 2), [0, 12], (32768, 65536, 0)), ((2, 0, 4), [4], (16384, 16384, 0)), ((0, 0, 1), [24], (16384, 49152, 0)),
                     ((1, 1, 2), [28], (16384, 16384, 0))]


def _row(lo, size, cell, S, n):
    """The header's expression in plain Python floats (IEEE double, one rounding per operation, in the order written)."""
    return [lo[k] + (float(cell[k]) + (float(S[k]) + 0.5 * float(n)) / (65536.0 * float(n))) * size for k in range(3)]


def _check_hand(out, voxels, lo, size, colors, np_t):
    xyz, color, cell, n, first, count = out
    assert count == len(voxels) and xyz.dtype == np_t and cell.dtype == n.dtype == first.dtype == np.int32
    assert cell.tolist() == [list(v[0]) for v in voxels] and n.tolist() == [len(v[1]) for v in voxels] and first.tolist() == [v[1][0] for v in voxels]
    want = np.array([_row(lo, size, c, S, len(m)) for c, m, S in voxels], np.float64)
    assert _bits(xyz, want.astype(np_t)), (xyz, want)
    if colors is not None:  # pixel i has the bytes (4 i .. 4 i + 3): the mean of channel j is (sum of 4 i + j) / n, rounded half up
        assert color.dtype == np.uint8
        assert color.tolist() == [[(2 * (4 * sum(m) + j * len(m)) + len(m)) // (2 * len(m)) for j in range(4)] for _, m, _ in voxels]
    else:
        assert color is None


def test_hand_built_map(sv):
    colors = np.arange(5 * 6 * 4, dtype=np.uint8).reshape(5, 6, 4)
    lo, hi = (-1.0, -1.0, 0.0), (11.0, 9.0, 24.0)
    assert sum(len(m) for _, m, _ in HAND_VOXELS) == 21
    for dtype, np_t in (("f32", np.float32), ("f64", np.float64)):
        _check_hand(sv.voxel_cloud(HAND_D, HAND_Q, 4.0, lo, hi, dtype=dtype, colors=colors), HAND_VOXELS, lo, 4.0, colors, np_t)
        _check_hand(sv.voxel_cloud(HAND_D, HAND_Q, 4.0, lo, hi, dtype=dtype, step=2), HAND_VOXELS_STEP2, lo, 4.0, None, np_t)
        # the 8-bit form: q = 4 d, so P is a quarter of the above (pixels 7 and 23, d = 0.125, have q = 0 - they were outside anyway); a
        # quarter of the crop and of the size gives the same t, cells and sums
        lo4, hi4 = (-0.25, -0.25, 0.0), (2.75, 2.25, 6.0)
        _check_hand(sv.voxel_cloud(HAND_D, HAND_Q, 1.0, lo4, hi4, dtype=dtype, disparity="dmap", colors=colors), HAND_VOXELS, lo4, 1.0, colors, np_t)
        _check_hand(sv.voxel_cloud(HAND_D, HAND_Q, 1.0, lo4, hi4, dtype=dtype, disparity="dmap", step=2), HAND_VOXELS_STEP2, lo4, 1.0, None, np_t)
    # a voxel of one point is that point moved by half an offset unit: size * 2^-17 = 2^-15 here, exactly
    xyz = sv.voxel_cloud(HAND_D, HAND_Q, 4.0, lo, hi, dtype="f64")[0]
    e = 2.0 ** -15
    assert xyz[3].tolist() == [8 + e, e, 16 + e] and xyz[5].tolist() == [e, 6 + e, 16 + e] and xyz[6].tolist() == [2 + e, 3 + e, 8 + e]
    # a transform, step 2: P' = (Z + .5, -X - .25, -Y + 2); crop (0.5, -11.25, -7) .. (24.5, 0.75, 3), size 4: t = (Z / 4, (11 - X) / 4, (9 - Y) / 4),
    # 6 x 3 x 3 cells; pixels 0, 4, 12, 24, 28 -> P = (0,0,8), (8,0,16), (0,2,8), (0,2,4), (4,4,8), each alone in its cell
    lo_t, hi_t = (0.5, -11.25, -7.0), (24.5, 0.75, 3.0)
    out = sv.voxel_cloud(HAND_D, HAND_Q, 4.0, lo_t, hi_t, XR=HAND_XR, XT=HAND_XT, step=2, dtype="f64", colors=colors)
    assert out[5] == 5 and out[4].tolist() == [0, 4, 12, 24, 28] and out[3].tolist() == [1] * 5
    assert out[2].tolist() == [[2, 2, 2], [4, 0, 2], [2, 2, 1], [1, 2, 1], [2, 1, 1]]
    assert out[0].tolist() == [[8.5 + e, -0.25 + e, 2 + e], [16.5 + e, -8.25 + e, 2 + e], [8.5 + e, -0.25 + e, e], [4.5 + e, -0.25 + e, e], [8.5 + e, -4.25 + e, -2 + e]]
    assert np.array_equal(out[1], colors.reshape(-1, 4)[[0, 4, 12, 24, 28]])  # the mean of one colour is that colour
    # a quotient that rounds onto the number of cells: X = 0.9 < hi = nextafter(0.9, 1), size 0.1: (hi - lo) / size = 9.0 cells, and
    # t = 0.9 / 0.1 = 9.0 too - the first min keeps the cell at 8, the second the offset at 65535
    hi_x = float(np.nextafter(0.9, 1.0))
    assert 0.9 < hi_x and 0.9 / 0.1 == 9.0 and hi_x / 0.1 == 9.0
    Q = np.array([[0.9, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 8], [0, 0, 1, 0]], np.float64)
    lo_r = (0.0, -1.0, 0.0)
    out = sv.voxel_cloud(np.array([[-16, 1]], np.float32), Q, 0.1, lo_r, (hi_x, 1.0, 16.0), dtype="f64")
    assert out[5] == 1 and out[2].tolist() == [[8, 10, 80]] and out[4].tolist() == [1]
    assert out[0][0].tolist() == _row(lo_r, 0.1, (8, 10, 80), (65535, 0, 0), 1) and out[0][0, 0] < hi_x
    # batched input: a list, one tuple per frame, each the frame's own
    two = sv.voxel_cloud(np.stack([HAND_D, HAND_D[::-1]]), HAND_Q, 4.0, lo, hi)
    assert len(two) == 2 and two[0][4].tolist() == [v[1][0] for v in HAND_VOXELS] and _bits(two[1][0], sv.voxel_cloud(HAND_D[::-1], HAND_Q, 4.0, lo, hi)[0])
    # capacity
    assert sv.voxel_cloud(HAND_D, HAND_Q, 4.0, lo, hi, capacity=9)[5] == 9
    over = sv.voxel_cloud(HAND_D, HAND_Q, 4.0, lo, hi, capacity=8, colors=colors)
    assert over[5] == -1 and over[0].shape == (0, 3) and over[1].shape == (0, 4) and over[3].shape == (0,)


BAD_GRIDS = [dict(size=0.0), dict(size=-1.0), dict(size=NAN), dict(size=INF), dict(lo=(-INF, 0, 0)), dict(hi=(1, INF, 1)), dict(lo=(NAN, 0, 0)),
             dict(lo=(0, 0, 0), hi=(1, 0, 1)), dict(lo=(0, 0, 2), hi=(1, 1, 1)), dict(lo=None), dict(hi=None), dict(hi=(1, 1)),
             dict(size=5e-7), dict(lo=(-1e308, 0, 0), hi=(1e308, 1, 1)),  # 1 / 5e-7 > 2^20 cells; hi - lo overflows
             dict(step=0), dict(step=1.5), dict(disparity="depth"), dict(dtype="f16"), dict(capacity=0), dict(capacity=2 ** 26 + 1), dict(capacity=1.5)]


def test_numpy_form_refuses_bad_arguments(sv):
    good = dict(size=0.5, lo=(0, 0, 0), hi=(1, 1, 1))
    assert sv.voxel_cloud(HAND_D, HAND_Q, **good)[5] >= 0
    for bad in BAD_GRIDS + [dict(colors=np.zeros((5, 6, 3), np.uint8)), dict(size="big")]:
        with pytest.raises(ValueError):
            sv.voxel_cloud(HAND_D, HAND_Q, **dict(good, **bad))
    with pytest.raises(ValueError):
        sv.voxel_cloud(np.zeros(5, np.float32), HAND_Q, **good)
    # exactly 2^20 cells are admitted, one more is not
    assert sv.voxel_grid(1.0, (0, 0, 0), (2 ** 20, 1, 1))[3].tolist() == [2 ** 20, 1, 1]
    with pytest.raises(ValueError):
        sv.voxel_grid(1.0, (0, 0, 0), (2 ** 20 + 0.5, 1, 1))
    assert [sv.voxel_table_slots(c) for c in (1, 512, 513, 1024, 1025, 2 ** 26)] == [1024, 1024, 2048, 2048, 4096, 2 ** 27]


@functools.lru_cache(maxsize=None)
def _golden():
    return util.golden_npz("kitti0_d128")["final1"].reshape(H, W).astype(np.float32)


def test_definition_against_an_independent_derivation(sv):
    """voxel_cloud on the golden KITTI map == compact_cloud's f64 list grouped here with np.unique on packed cells; the means agree with
    float means within a derived bound."""
    d = _golden()
    rng = np.random.default_rng(41)
    colors = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    lo, hi = np.array(CLI_LO), np.array(CLI_HI)
    assert (d > 0).sum() == 465131
    P, col, index = sv.compact_cloud(d, KITTI_Q, XR=C2V, lo=CLI_LO, hi=CLI_HI, dtype="f64", colors=colors)
    assert len(index) == 143161  # the issue's figure for this map, Q and crop: the set-up is the one it measured
    for size, voxels in ((0.05, 45501), (0.1, 21427), (0.2, 8289), (0.5, 1867)):
        xyz, color, cell, n, first, count = sv.voxel_cloud(d, KITTI_Q, size, CLI_LO, CLI_HI, XR=C2V, dtype="f64", colors=colors)
        cells = np.maximum(np.ceil((hi - lo) / size), 1).astype(np.int64)
        c = np.minimum(np.floor((P - lo) / size).astype(np.int64), cells - 1)  # floor == truncation: the quotient is positive
        packed = (c[:, 2] * cells[1] + c[:, 1]) * cells[0] + c[:, 0]  # another packing than the definition's
        _, where, inverse, number = np.unique(packed, return_index=True, return_inverse=True, return_counts=True)
        order = np.argsort(index[where], kind="stable")
        assert count == len(where) == voxels and len(xyz) == count
        assert np.array_equal(first, index[where][order]) and np.array_equal(n, number[order]) and np.array_equal(cell, c[where][order])
        assert (np.diff(first) > 0).all() and n.sum() == len(index) and n.min() >= 1
        mean = np.zeros((len(where), 3))
        np.add.at(mean, inverse.reshape(-1), P)
        mean = (mean / number[:, None])[order]
        # |xyz - mean|: the definition truncates each offset to 1/65536 of the cell and adds half a unit back, so its mean is within
        # size * 2^-17 of the true one.  Rounding: the comparison mean is a recursive float64 sum of n terms of magnitude <= M =
        # max(|lo|, |hi|), error <= (n - 1) * 2^-53 * n M on the sum, i.e. (n - 1) * 2^-53 * M on the mean, plus one division; the
        # definition's side rounds (P - lo), the quotient, the product with 65536 (exact), the final quotient, two sums and a product,
        # each relative 2^-53 of a value <= M + size: 8 * 2^-53 * M covers them.  Together (n + 8) * 2^-53 * M.
        M = np.maximum(np.abs(lo), np.abs(hi))
        bound = size * 2.0 ** -17 + (n[:, None] + 8) * 2.0 ** -53 * M[None]
        err = np.abs(xyz - mean)
        print("size %.2f: %d voxels, points per voxel %.1f / %d, worst error / bound %.3f" % (size, count, n.mean(), n.max(), (err / bound).max()))
        assert (err <= bound).all(), (size, (err / bound).max())
        assert ((xyz > lo) & (xyz < hi)).all()  # a centroid lies inside its cell, so inside the crop
        fmean = np.zeros((len(where), 4))
        np.add.at(fmean, inverse.reshape(-1), col.astype(np.float64))
        fmean = (fmean / number[:, None])[order]
        assert (np.abs(color.astype(np.float64) - np.rint(fmean)) <= 1).all() and (np.abs(color - fmean) <= 0.5 + 1e-9).all()
        with np.errstate(over="ignore"):
            assert _bits(sv.voxel_cloud(d, KITTI_Q, size, CLI_LO, CLI_HI, XR=C2V, colors=colors)[0], xyz.astype(np.float32))


def test_one_point_per_voxel_and_one_voxel(sv):
    d = _golden()
    colors = np.random.default_rng(43).integers(0, 256, (H, W, 4), dtype=np.uint8)
    P, col, index = sv.compact_cloud(d, KITTI_Q, XR=C2V, lo=CLI_LO, hi=CLI_HI, dtype="f64", colors=colors, step=2)
    size = 40.0 / 2 ** 20  # the smallest size the crop admits: 2^20 cells ahead
    xyz, color, cell, n, first, count = sv.voxel_cloud(d, KITTI_Q, size, CLI_LO, CLI_HI, XR=C2V, dtype="f64", colors=colors, step=2)
    assert count == len(index) > 30000 and (n == 1).all(), (count, len(index))  # every kept point alone in its cell
    assert np.array_equal(first, index) and np.array_equal(color, col)
    # the point itself within size * 2^-17 and the roundings of the definition's side (the bound of the test above with n = 1)
    M = np.maximum(np.abs(CLI_LO), np.abs(CLI_HI))
    assert (np.abs(xyz - P) <= size * 2.0 ** -17 + 9 * 2.0 ** -53 * M).all()
    one = sv.voxel_cloud(d, KITTI_Q, 40.0, CLI_LO, CLI_HI, XR=C2V, colors=colors, step=2)  # one cell covers the crop
    assert one[5] == 1 and one[3].tolist() == [len(index)] and one[2].tolist() == [[0, 0, 0]] and one[4].tolist() == [int(index[0])]
    # capacity: V <= capacity gives V, capacity = V - 1 gives -1
    V = sv.voxel_cloud(d, KITTI_Q, 0.5, CLI_LO, CLI_HI, XR=C2V)[5]
    assert V == 1867 and sv.voxel_cloud(d, KITTI_Q, 0.5, CLI_LO, CLI_HI, XR=C2V, capacity=V)[5] == V
    assert sv.voxel_cloud(d, KITTI_Q, 0.5, CLI_LO, CLI_HI, XR=C2V, capacity=V - 1)[5] == -1


def _spec(eng, lo=(0.0, -20.0, -1.4), hi=(40.0, 20.0, 1.0), size=0.1, disparity=1, step=1, dtype=0, reserved=None):
    sp = eng.SvVoxelSpec()
    sp.lo[:], sp.hi[:] = lo, hi
    sp.size, sp.disparity, sp.step, sp.dtype = size, disparity, step, dtype
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


def _bad_specs(eng):
    return ([_spec(eng, reserved=k) for k in range(5)] + [_spec(eng, disparity=v) for v in (2, -1)] + [_spec(eng, dtype=v) for v in (2, -1)] +
            [_spec(eng, step=v) for v in (0, -3)] + [_spec(eng, size=v) for v in (0.0, -0.5, NAN, INF, 1e-6)] +
            [_spec(eng, lo=lo, hi=hi) for lo, hi in (((0, 0, 0), (1, 0, 1)), ((0, 0, 2), (1, 1, 1)), ((NAN, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, NAN, 1)),
                                                     ((-INF, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, INF)), ((-1e308, 0, 0), (1e308, 1, 1)))])


def test_validation_needs_no_device(eng):
    """Every SV_ERR_ARG case on host buffers: the checks run before any HIP call, so nothing is read or written; batch == 0 returns
    SV_OK with nothing enqueued.  The workspace size follows the documented layout, SIZE_MAX for bad input."""
    L = eng.voxel_lib()
    for name in ("sv_voxel_disparity_device", "sv_voxel_workspace_bytes", "sv_voxel_table_slots", "sv_debug_voxel"):
        assert hasattr(L, name)
    assert [L.sv_voxel_table_slots(c) for c in (1, 512, 513, 70000, 2 ** 26)] == [1024, 1024, 2048, 2 ** 18, 2 ** 27]
    assert [L.sv_voxel_table_slots(c) for c in (0, -1, 2 ** 26 + 1)] == [-1] * 3
    ws = lambda sp, b, w, h, cap: L.sv_voxel_workspace_bytes(ctypes.byref(sp) if sp is not None else None, b, w, h, cap)  # noqa: E731
    T = eng.cloud_tile()

    def expect(b, visited, cap):  # table + 16 bytes + the mask padded to 16 bytes, per pair; 4 bytes per tile and pair
        return b * (L.sv_voxel_table_slots(cap) * 72 + 16 + -(-(-(-visited // 32) * 4) // 16) * 16 + 4 * -(-visited // T))
    assert ws(_spec(eng), 2, 16, 8, 100) == expect(2, 128, 100) and ws(_spec(eng), 0, 16, 8, 100) == 0
    assert ws(_spec(eng), 3, W, H, 30000) == expect(3, W * H, 30000) and ws(_spec(eng, step=3), 3, W, H, 1) == expect(3, 414 * 125, 1)
    for sp in _bad_specs(eng) + [None]:
        assert ws(sp, 2, 16, 8, 100) == SIZE_MAX
    for b, w, h, cap in ((-1, 16, 8, 9), (65536, 16, 8, 9), (2, 0, 8, 9), (2, 16, 0, 9), (2, 65536, 32768, 9), (2, 16, 8, 0), (2, 16, 8, -4), (2, 16, 8, 2 ** 26 + 1)):
        assert ws(_spec(eng), b, w, h, cap) == SIZE_MAX
    nbytes = ws(_spec(eng), 2, 16, 8, 128)
    bufs = {k: np.full(8192, 0x5A, np.uint8) for k in ("disp", "colors", "xyz", "color_out", "cell", "n", "first", "counts")}
    bufs["ws"] = np.full(nbytes + 64, 0x5A, np.uint8)
    bufs["Q"] = np.eye(4).reshape(16)
    ptr = lambda name: bufs[name].ctypes.data + (-bufs[name].ctypes.data % 16 if name == "ws" else 0)  # noqa: E731
    good = dict(disp=ptr("disp"), colors=ptr("colors"), batch=2, width=16, height=8, Q=ptr("Q"), XR=None, XT=None, spec=_spec(eng), capacity=128,
                xyz=ptr("xyz"), color_out=ptr("color_out"), cell=ptr("cell"), n=ptr("n"), first=ptr("first"), counts=ptr("counts"), ws=ptr("ws"),
                ws_bytes=nbytes)

    def call(**kw):
        a = dict(good, **kw)
        sp = ctypes.byref(a["spec"]) if a["spec"] is not None else None
        return L.sv_voxel_disparity_device(a["disp"], a["colors"], a["batch"], a["width"], a["height"], a["Q"], a["XR"], a["XT"], sp, a["capacity"], a["xyz"],
                                           a["color_out"], a["cell"], a["n"], a["first"], a["counts"], a["ws"], a["ws_bytes"], None)

    cases = [dict(spec=None), dict(disp=None), dict(Q=None), dict(counts=None), dict(xyz=None), dict(colors=None), dict(capacity=0), dict(capacity=-1),
             dict(capacity=2 ** 26 + 1), dict(batch=-1), dict(batch=65536), dict(width=0), dict(height=0), dict(width=-5), dict(width=65536, height=32768),
             dict(width=46341, height=46341), dict(ws=None), dict(ws_bytes=nbytes - 1), dict(ws_bytes=0), dict(ws=ptr("ws") + 8),
             dict(colors=ptr("colors") + 1), dict(color_out=ptr("color_out") + 2)]
    cases += [dict(spec=sp) for sp in _bad_specs(eng)]
    assert len(cases) == 22 + 23
    for kw in cases:
        rc = call(**kw)
        text = L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_voxel"), (sorted(kw), rc, text)
    assert call(batch=0) == 0 and call(batch=0, ws=None, ws_bytes=0) == 0
    assert all((bufs[k] == 0x5A).all() for k in bufs if k != "Q")
    good_kw = dict(size=0.1, lo=CLI_LO, hi=CLI_HI)
    for bad in BAD_GRIDS:
        with pytest.raises(ValueError):
            eng.voxel_spec(**dict(good_kw, **bad))
    sp = eng.voxel_spec(0.25, CLI_LO, CLI_HI, step=3, disparity="dmap", dtype="f64")
    assert (list(sp.lo), list(sp.hi), sp.size, sp.disparity, sp.step, sp.dtype, list(sp.reserved)) == (list(CLI_LO), list(CLI_HI), 0.25, 0, 3, 1, [0] * 5)
    assert ctypes.sizeof(sp) == 88


def test_write_ply_takes_a_voxel_cloud(sv, tmp_path):
    colors = np.random.default_rng(47).integers(0, 256, (H, W, 4), dtype=np.uint8)
    out = sv.voxel_cloud(_golden(), KITTI_Q, 0.2, CLI_LO, CLI_HI, XR=C2V, colors=colors)
    sv.write_ply(tmp_path / "v.ply", *out[:2])
    head, payload = _read_ply(tmp_path / "v.ply")
    rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert head[2] == "element vertex 8289" and rec.shape == (8289,)
    assert _bits(rec["xyz"], out[0]) and np.array_equal(rec["rgb"], out[1][:, 2::-1])
    sv.write_ply(tmp_path / "p.ply", sv.voxel_cloud(_golden(), KITTI_Q, 0.5, CLI_LO, CLI_HI, XR=C2V)[0])
    assert _read_ply(tmp_path / "p.ply")[0][2] == "element vertex 1867"


# ---------------------------------------------------------------------------------------------------------------- GPU

def _gpu(eng, d, Q, size, lo, hi, colors=None, **kw):
    """The engine call on numpy inputs -> (per-frame (xyz, color or None, cell, n, first) or None for an overflowed frame, counts)."""
    d = np.asarray(d, np.float32)
    d = d[None] if d.ndim == 2 else d
    if colors is not None:
        colors = _cuda(colors[None] if colors.ndim == 3 else colors)
    xyz, color, cell, n, first, counts = eng.voxel_cloud_from_disparity(_cuda(d), Q, size, lo, hi, colors=colors, want_cell=True, want_first=True, **kw)
    assert xyz.is_cuda and counts.is_cuda and tuple(counts.shape) == (d.shape[0],)
    k = counts.cpu().numpy()
    cut = lambda t, b: None if t is None else t[b, :k[b]].cpu().numpy()  # noqa: E731
    return [None if k[b] < 0 else tuple(cut(t, b) for t in (xyz, color, cell, n, first)) for b in range(d.shape[0])], k


def _same(got, want):
    return got is not None and all((g is None) == (w is None) and (g is None or _bits(g, w)) for g, w in zip(got, want[:5]))


def _check(sv, eng, d, Q, size, lo, hi, colors=None, want=None, **kw):
    """GPU == definition, bit for bit, for every frame of d; returns the counts."""
    d = np.asarray(d, np.float32)
    d = d[None] if d.ndim == 2 else d
    got, counts = _gpu(eng, d, Q, size, lo, hi, colors, **kw)
    if want is None:
        want = sv.voxel_cloud(d, Q, size, lo, hi, colors=colors if colors is None or colors.ndim == 4 else colors[None], **kw)
    assert len(got) == len(want) == d.shape[0]
    for b, (g, w) in enumerate(zip(got, want)):
        assert counts[b] == w[5], (b, counts[b], w[5], size, kw)
        assert w[5] < 0 or _same(g, w), (b, size, kw)
    return counts


XFS = {"none": (None, None, CAM_LO, CAM_HI), "vehicle": (C2V, None, CLI_LO, CLI_HI)}


@functools.lru_cache(maxsize=None)
def _kitti_colors():
    return np.random.default_rng(17).integers(0, 256, (3, H, W, 4), dtype=np.uint8)


_defined = {}


def _kitti_defined(sv, d1, Q, kind, step, size, xf):
    key = (kind, step, size, xf)
    if key not in _defined:
        XR, XT, lo, hi = XFS[xf]
        _defined[key] = sv.voxel_cloud(d1, Q, size, lo, hi, XR=XR, XT=XT, step=step, disparity=kind, dtype="f64", colors=_kitti_colors())
    return _defined[key]


@pytest.mark.gpu
@pytest.mark.parametrize("with_colors", [True, False])
@pytest.mark.parametrize("xf", list(XFS))
@pytest.mark.parametrize("size", [0.05, 0.2, 1.0])
@pytest.mark.parametrize("step", [1, 2, 3])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["dmap", "d1"])
def test_fused_equals_definition(sv, eng, kitti_d1, kind, dtype, step, size, xf, with_colors):
    d1, Q = kitti_d1
    XR, XT, lo, hi = XFS[xf]
    want = _kitti_defined(sv, d1, Q, kind, step, size, xf)
    if dtype == "f32":  # the definition's float32 form is astype(float32) of these doubles (checked against voxel_cloud itself below)
        want = [(w[0].astype(np.float32),) + w[1:] for w in want]
        if (step, size, xf, with_colors) == (3, 0.2, "vehicle", True):
            direct = sv.voxel_cloud(d1, Q, size, lo, hi, XR=XR, XT=XT, step=step, disparity=kind)
            assert all(_bits(a[0], b[0]) for a, b in zip(direct, want))
    if not with_colors:
        want = [(w[0], None) + w[2:] for w in want]
    counts = _check(sv, eng, d1, Q, size, lo, hi, _kitti_colors() if with_colors else None, want=want, XR=XR, XT=XT, step=step, disparity=kind, dtype=dtype,
                    capacity=None if size == 0.2 else 200000)
    assert counts.min() > (0 if kind == "dmap" else 100), counts  # the quarter-depth cloud fills few cells of a metric crop


BIG_LO, BIG_HI = (-50.0, -30.0, 1.0), (50.0, 30.0, 200.0)


@pytest.mark.gpu
def test_shapes_around_the_tiling(sv, eng):
    T = eng.cloud_tile()
    rng = np.random.default_rng(23)
    shapes = [(1, 1), (1, 70), (70, 1), (5, 63), (5, 64), (5, 65), (3, 1241), (1, T - 1), (1, T), (1, T + 1), (1, 4 * T - 1), (1, 4 * T), (1, 4 * T + 1),
              (7, 4 * T + 3)]
    for h, w in shapes:
        d = _random_map(rng, h, w, 0.7)
        colors = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        for kind, dtype, size in (("d1", "f32", 0.5), ("dmap", "f64", 2.0)):
            _check(sv, eng, d, SMALL_Q, size, BIG_LO, BIG_HI, colors, disparity=kind, dtype=dtype)
        _check(sv, eng, d, SMALL_Q, 5.0, BIG_LO, BIG_HI, colors, step=2)
    for n in (T - 1, T, T + 1):  # the visited lattice, not the image, is what is tiled
        d = _random_map(rng, 4, 3 * n - 2, 0.6)
        _check(sv, eng, d, SMALL_Q, 1.0, BIG_LO, BIG_HI, step=3)
    d = _random_map(rng, 40, 50, 1.0)
    for step in (50, 1000, 2 ** 31 - 1):  # pixel (0, 0) alone is visited
        assert _check(sv, eng, d, SMALL_Q, 1.0, (-1000, -1000, 0), (1000, 1000, 2000), step=step, dtype="f64").tolist() == [1]
    for density in (0.0, 0.01, 0.3, 1.0):  # random maps of several densities; frames whose rows do not start on 16 bytes
        maps = np.stack([_random_map(rng, 9, 333, density) for _ in range(4)])
        counts = _check(sv, eng, maps, SMALL_Q, 2.0, BIG_LO, BIG_HI, rng.integers(0, 256, (4, 9, 333, 4), dtype=np.uint8))
        assert (counts == 0).all() == (density == 0.0)


@pytest.mark.gpu
def test_a_4k_frame(sv, eng):
    rng = np.random.default_rng(29)
    d = _random_map(rng, 2160, 3840, 0.8)
    Q = np.array([[1, 0, 0, -1920.0], [0, 1, 0, -1080.0], [0, 0, 0, 2800.0], [0, 0, 1 / 0.3, 0]], np.float64)
    colors = rng.integers(0, 256, (2160, 3840, 4), dtype=np.uint8)
    counts = _check(sv, eng, d, Q, 1.0, (-40, -20, 0.5), (40, 20, 60.0), colors, capacity=2 ** 18)  # 80 x 40 x 60 = 192 000 cells
    assert 50000 < counts[0] <= 192000


def _counters(eng, combine, fn):
    """fn() under sv_debug_voxel(combine, counters) -> (fn's result, table updates, atomic instructions)."""
    import torch
    c = torch.zeros(2, dtype=torch.int64, device="cuda")
    try:
        eng.debug_voxel(combine, c)
        out = fn()
        torch.cuda.synchronize()
    finally:
        eng.debug_voxel(True, None)
    return out, int(c[0].item()), int(c[1].item())


@pytest.mark.gpu
def test_contention_and_the_combine_hook(sv, eng, kitti_d1):
    d1, Q = kitti_d1
    colors = _kitti_colors()
    kept = [len(f[2]) for f in sv.compact_cloud(d1, Q, XR=C2V, lo=CLI_LO, hi=CLI_HI)]
    alone = 40.0 / 2 ** 20
    for size, capacity in ((40.0, 512), (0.1, 65536), (alone, None)):  # all points in ONE voxel ... every point (nearly) in its own
        want = sv.voxel_cloud(d1, Q, size, CLI_LO, CLI_HI, XR=C2V, colors=colors)
        if size == 40.0:
            assert [w[5] for w in want] == [1, 1, 1] and [int(w[3][0]) for w in want] == kept
        if size == alone:
            assert all(w[5] > 0.99 * k for w, k in zip(want, kept))
        res = {}
        for combine in (True, False):
            (got, counts), updates, atomics = _counters(eng, combine, lambda: _gpu(eng, d1, Q, size, CLI_LO, CLI_HI, colors, XR=C2V, capacity=capacity))
            assert counts.tolist() == [w[5] for w in want] and all(_same(g, w) for g, w in zip(got, want)), (size, combine)
            res[combine] = (updates, atomics)
        print("size %g: %d points; table updates %d combined / %d not; atomic instructions %d / %d" % (
            size, sum(kept), res[True][0], res[False][0], res[True][1], res[False][1]))
        assert res[False][0] == sum(kept)  # without the merge one update per kept point
        if size != alone:  # strictly fewer with it on the KITTI maps; nothing to merge where every point has its own cell
            assert res[True][0] < sum(kept) and res[True][1] < res[False][1]
        assert res[True][0] <= sum(kept) and res[True][1] <= res[False][1]


def _raw(eng, d_t, colors_t, Q, spec, capacity, xyz, color, cell, n, first, counts, XR=None, ws=None, stream=None):
    """The C entry on caller-owned buffers (torch tensors); the workspace is the caller's too when given."""
    import torch
    L = eng.voxel_lib()
    B, Hh, Ww = d_t.shape
    nbytes = L.sv_voxel_workspace_bytes(ctypes.byref(spec), B, Ww, Hh, capacity)
    assert nbytes != SIZE_MAX
    if ws is None:
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= nbytes and ws.data_ptr() % 16 == 0
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = L.sv_voxel_disparity_device(d_t.data_ptr(), ptr(colors_t), B, Ww, Hh, q.ctypes.data, None if XR is None else XR.ctypes.data, None, ctypes.byref(spec),
                                     capacity, ptr(xyz), ptr(color), ptr(cell), ptr(n), ptr(first), counts.data_ptr(), ws.data_ptr(), nbytes,
                                     torch.cuda.current_stream().cuda_stream if stream is None else stream)
    assert rc == 0, (rc, L.sv_last_error(None))
    return ws


@pytest.mark.gpu
def test_capacity_edges(sv, eng, kitti_d1):
    import torch
    d1, Q = kitti_d1
    colors = _kitti_colors()
    kw = dict(XR=C2V)
    want = sv.voxel_cloud(d1, Q, 0.2, CLI_LO, CLI_HI, colors=colors, **kw)
    V = [w[5] for w in want]
    assert min(V) > 1000 and len(set(V)) == 3
    t, c = _cuda(d1), _cuda(colors)
    spec = eng.voxel_spec(0.2, CLI_LO, CLI_HI)
    xr = np.ascontiguousarray(C2V)
    order = sorted(V)
    for cap in (order[0] - 1, order[0], order[1] - 1, order[1], order[2] - 1, order[2], order[2] + 7):  # V == capacity, V == capacity + 1; some frames over
        xyz = torch.full((3, cap, 3), -7.25, dtype=torch.float32, device="cuda")
        col = torch.full((3, cap, 4), 0x5A, dtype=torch.uint8, device="cuda")
        cell = torch.full((3, cap, 3), -77, dtype=torch.int32, device="cuda")
        n = torch.full((3, cap), -77, dtype=torch.int32, device="cuda")
        first = torch.full((3, cap), -77, dtype=torch.int32, device="cuda")
        counts = torch.full((3,), -5, dtype=torch.int32, device="cuda")
        _raw(eng, t, c, Q, spec, cap, xyz, col, cell, n, first, counts, XR=xr)
        torch.cuda.synchronize()
        assert counts.tolist() == [v if v <= cap else -1 for v in V], (cap, counts.tolist(), V)
        for b in range(3):
            k = V[b] if V[b] <= cap else 0  # an overflowed frame's rows are untouched, the others are unaffected by it
            got = tuple(x[b, :k].cpu().numpy() for x in (xyz, col, cell, n, first))
            assert all(_bits(g, w[:k]) for g, w in zip(got, want[b][:5])), (cap, b)
            assert (xyz[b, k:] == -7.25).all().item() and (col[b, k:] == 0x5A).all().item() and all((x[b, k:] == -77).all().item() for x in (cell, n, first))
    # the engine layer: counts -1, and the cutter refuses to slice with it
    out = eng.voxel_cloud_from_disparity(t, Q, 0.2, CLI_LO, CLI_HI, colors=c, capacity=order[1], **kw)
    assert sorted(out[5].tolist()) == [-1, order[0], order[1]]
    with pytest.raises(eng.StereoError):
        eng.split_voxel_clouds(out[0], out[5], out[1])
    for bad in (0, -1, 1.5, 2 ** 26 + 1):
        with pytest.raises(ValueError):
            eng.voxel_cloud_from_disparity(t, Q, 0.2, CLI_LO, CLI_HI, capacity=bad)


@pytest.mark.gpu
def test_batches_and_repeats(sv, eng, kitti_d1):
    import torch
    d1, Q = kitti_d1
    rng = np.random.default_rng(37)
    frames = np.stack([d1[0], d1[1], d1[2], _random_map(rng, H, W, 0.3), np.where(d1[0] > 20, d1[0], np.float32(-10))])
    colors = rng.integers(0, 256, (5, H, W, 4), dtype=np.uint8)
    lo, hi = (-5.0, -30.0, -2.0), (60.0, 30.0, 4.0)
    kw = dict(XR=XR_G, XT=XT_G, step=2, capacity=60000)
    batch, counts = _gpu(eng, frames, Q, 0.15, lo, hi, colors, **kw)
    assert len(set(counts.tolist())) == 5 and counts.min() > 0
    want = sv.voxel_cloud(frames, Q, 0.15, lo, hi, colors=colors, **kw)
    assert all(_same(g, w) for g, w in zip(batch, want))
    # a frame alone, and at every position of a batch of 5
    for b in range(5):
        alone, n = _gpu(eng, frames[b], Q, 0.15, lo, hi, colors[b], **kw)
        assert n[0] == counts[b] and _same(alone[0], batch[b])
    for shift in range(1, 5):
        rolled, n = _gpu(eng, np.roll(frames, shift, 0), Q, 0.15, lo, hi, np.roll(colors, shift, 0), **kw)
        assert np.array_equal(n, np.roll(counts, shift)) and all(_same(rolled[(b + shift) % 5], batch[b]) for b in range(5))
    # 5 repeated calls on one dirty workspace: an accumulator that depended on the order, or on what the workspace held, would differ
    spec = eng.voxel_spec(0.15, lo, hi, step=2)
    t, c = _cuda(frames), _cuda(colors)
    nbytes = eng.voxel_lib().sv_voxel_workspace_bytes(ctypes.byref(spec), 5, W, H, 60000)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    xr = np.ascontiguousarray(XR_G)
    for rep in range(5):
        bufs = (torch.zeros((5, 60000, 3), dtype=torch.float32, device="cuda"), torch.zeros((5, 60000, 4), dtype=torch.uint8, device="cuda"),
                torch.zeros((5, 60000, 3), dtype=torch.int32, device="cuda"), torch.zeros((5, 60000), dtype=torch.int32, device="cuda"),
                torch.zeros((5, 60000), dtype=torch.int32, device="cuda"))
        n = torch.zeros((5,), dtype=torch.int32, device="cuda")
        L = eng.voxel_lib()
        q = np.ascontiguousarray(Q, np.float64).reshape(16)
        rc = L.sv_voxel_disparity_device(t.data_ptr(), c.data_ptr(), 5, W, H, q.ctypes.data, xr.ctypes.data, XT_G.ctypes.data, ctypes.byref(spec), 60000,
                                         bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), n.data_ptr(),
                                         ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(n.cpu().numpy(), counts)
        for b in range(5):
            assert _same(tuple(x[b, :counts[b]].cpu().numpy() for x in bufs), batch[b]), (rep, b)
    # an empty batch: nothing is enqueued, empty outputs
    out = eng.voxel_cloud_from_disparity(torch.empty((0, 8, 16), device="cuda"), Q, 0.5, lo, hi)
    assert tuple(out[0].shape) == (0, 128, 3) and out[1] is None and tuple(out[5].shape) == (0,) and eng.split_voxel_clouds(out[0], out[5]) == []
    # 300 small frames
    small = np.stack([_random_map(rng, 23, 41, 0.6) for _ in range(300)])
    counts = _check(sv, eng, small, SMALL_Q, 4.0, BIG_LO, BIG_HI, rng.integers(0, 256, (300, 23, 41, 4), dtype=np.uint8), dtype="f64", capacity=1000)
    assert len(set(counts.tolist())) > 10 and counts.min() > 0
    # input checks of the engine layer
    td = _cuda(d1)
    for bad in (dict(d1=td.double()), dict(d1=td.cpu()), dict(colors=_cuda(colors[:3, :, :, :3])), dict(colors=_cuda(colors[:2])), dict(colors=colors[:3]),
                dict(step=0), dict(disparity="depth"), dict(dtype="f16"), dict(hi=(60, 30, -2)), dict(size=0), dict(lo=None)):
        with pytest.raises(ValueError):
            eng.voxel_cloud_from_disparity(**dict(dict(d1=td, Q=Q, size=0.15, lo=lo, hi=hi), **bad))


@pytest.mark.gpu
def test_optional_outputs_and_torch_stream(sv, eng, kitti_d1):
    """An output left out does not change the others; inputs written by torch ops on a busy side stream and a dependent torch op behind
    the call, no explicit synchronisation in between: the results are those of the inputs at rest."""
    import torch
    d1, Q = kitti_d1
    colors = _kitti_colors()
    t, c = _cuda(d1), _cuda(colors)
    kw = dict(XR=C2V, capacity=30000)
    full = eng.voxel_cloud_from_disparity(t, Q, 0.2, CLI_LO, CLI_HI, colors=c, want_cell=True, want_n=True, want_first=True, **kw)
    k = full[5].cpu().numpy()
    assert k.min() > 1000
    for flags in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        for with_colors in (True, False):
            part = eng.voxel_cloud_from_disparity(t, Q, 0.2, CLI_LO, CLI_HI, colors=c if with_colors else None, want_cell=flags[0], want_n=flags[1],
                                                  want_first=flags[2], **kw)
            assert torch.equal(part[5], full[5]) and [x is not None for x in part[1:5]] == [with_colors] + list(flags)
            for b in range(3):
                assert all(x is None or _bits(x[b, :k[b]].cpu().numpy(), f[b, :k[b]].cpu().numpy()) for x, f in zip(part[:5], full[:5]))
    src_d, src_c = _cuda(d1), _cuda(colors)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):
            x = x @ x  # keeps the stream busy while the host runs ahead
        d = torch.zeros_like(src_d)
        d.copy_(src_d)
        cc = torch.zeros_like(src_c)
        cc.copy_(src_c)
        out = eng.voxel_cloud_from_disparity(d, Q, 0.2, CLI_LO, CLI_HI, colors=cc, want_cell=True, want_first=True, **kw)
        total = out[5].sum()  # dependent ops on the same stream
        heads = torch.stack([out[0][b, 0] for b in range(3)]) * 2
    torch.cuda.synchronize()
    del x
    assert torch.equal(out[5], full[5]) and total.item() == k.sum()
    for b in range(3):
        assert all(_bits(g[b, :k[b]].cpu().numpy(), f[b, :k[b]].cpu().numpy()) for g, f in zip(out[:5], full[:5]))
    assert _bits(heads.cpu().numpy(), np.stack([full[0][b, 0].cpu().numpy() for b in range(3)]) * 2)


@pytest.mark.gpu
def test_rig_voxel_clouds(sv, eng):
    import torch
    rigmod = util.pkg("rig")
    bgr_l, bgr_r = _colour_pairs()
    kw = dict(transform=(sv.CAMERA_TO_VEHICLE, None), capacity=50000)
    rig = rigmod.StereoRig(W, H)
    try:
        tl, tr = _cuda(bgr_l), _cuda(bgr_r)
        xyz, color, n, counts = rig.voxel_clouds(tl, tr, 0.1, CLI_LO, CLI_HI, **kw)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (xyz, color, n, counts)) and tuple(xyz.shape) == (2, 50000, 3) and xyz.dtype == torch.float32
        d1 = rig.disparity(tl, tr)
        col = rig.frontend(tl, tr, colors=True)[2]
        want = sv.voxel_cloud(d1.cpu().numpy(), rig.Q, 0.1, CLI_LO, CLI_HI, XR=sv.CAMERA_TO_VEHICLE, colors=col.cpu().numpy())
        k = counts.cpu().numpy()
        assert k.tolist() == [w[5] for w in want] and k.min() > 5000
        frames = rig.voxel_clouds(bgr_l, bgr_r, 0.1, CLI_LO, CLI_HI, **kw)  # numpy in: per-frame numpy arrays
        assert isinstance(frames, list) and len(frames) == 2
        for b, (p, c, m) in enumerate(frames):
            assert all(isinstance(x, np.ndarray) for x in (p, c, m)) and p.shape == (k[b], 3)
            assert _bits(p, want[b][0]) and np.array_equal(c, want[b][1]) and np.array_equal(m, want[b][3])
            assert _bits(p, xyz[b, :k[b]].cpu().numpy()) and np.array_equal(c, color[b, :k[b]].cpu().numpy()) and np.array_equal(m, n[b, :k[b]].cpu().numpy())
        p2, c2, n2, k2 = rig.voxel_clouds(tl, tr, 0.5, CLI_LO, CLI_HI, transform=(sv.CAMERA_TO_VEHICLE, None), colors=False, dtype="f64", step=2)
        want2 = sv.voxel_cloud(d1.cpu().numpy(), rig.Q, 0.5, CLI_LO, CLI_HI, XR=sv.CAMERA_TO_VEHICLE, dtype="f64", step=2)
        assert c2 is None and p2.dtype == torch.float64 and tuple(p2.shape) == (2, 621 * 188, 3)
        assert all(k2[b].item() == want2[b][5] and _bits(p2[b, :want2[b][5]].cpu().numpy(), want2[b][0]) for b in range(2))
        with pytest.raises(eng.StereoError):  # numpy in cuts the frames, and a frame over the capacity cannot be cut
            rig.voxel_clouds(bgr_l, bgr_r, 0.1, CLI_LO, CLI_HI, transform=(sv.CAMERA_TO_VEHICLE, None), capacity=100)
        for bad in (dict(size=0), dict(lo=None), dict(hi=(40, 20, INF)), dict(step=0), dict(dtype="f16"), dict(transform="sideways"), dict(capacity=0)):
            with pytest.raises(ValueError):
                rig.voxel_clouds(bgr_l, bgr_r, **dict(dict(size=0.1, lo=CLI_LO, hi=CLI_HI), **bad))
    finally:
        rig.close()


@pytest.mark.gpu
def test_cli_voxel_ply(sv, tmp_path):
    from PIL import Image
    for d in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / d)
    bgr_l, bgr_r = _colour_pairs(3, seed=3)
    for i in range(3):
        Image.fromarray(bgr_l[i][..., ::-1]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(bgr_r[i][..., ::-1]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with pytest.raises(SystemExit):
        sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--voxel", "0.2"])  # needs --ply
    with pytest.raises(SystemExit):
        sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply"), "--voxel", "-1"])
    sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply"), "--voxel", "0.2"])
    rig = util.pkg("rig").StereoRig(W, H)
    try:
        xyz, color, n, counts = rig.voxel_clouds(_cuda(bgr_l), _cuda(bgr_r), 0.2, sv.CLI_CLOUD_CROP[0], sv.CLI_CLOUD_CROP[1], transform=(sv.CAMERA_TO_VEHICLE, None))
    finally:
        rig.close()
    k = counts.cpu().numpy()
    for i in range(3):
        head, payload = _read_ply(tmp_path / "ply" / ("%010d.ply" % i))
        rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
        assert head[2] == "element vertex %d" % k[i] and k[i] > 1000
        assert _bits(rec["xyz"], xyz[i, :k[i]].cpu().numpy()) and np.array_equal(rec["rgb"], color[i, :k[i]].cpu().numpy()[:, 2::-1])
