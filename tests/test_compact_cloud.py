"""Compact coloured point clouds (include/stereo_vision_hip.h (F)): the numpy restatement stereo_vision.sv.compact_cloud on a hand-built
map and against an independently written mask over the dense cloud, the C ABI's argument checks, write_ply, and the HIP kernels - C
entry, engine and rig layers - against the restatement.

Everything is compared bitwise (integer views of the floats) and the counts exactly: a kept point passed a strict comparison on every
axis, so it holds no NaN, and the float32 form is IEEE round-to-nearest-even of the same doubles on both sides."""
import ctypes
import functools
import os

import numpy as np
import pytest

import util
from test_top_view import _cuda, _reproject_np, eng, kitti_d1, sv  # noqa: F401 (fixtures)

SV_ERR_ARG = -1
SIZE_MAX = 2 ** 64 - 1
NAN, INF = float("nan"), float("inf")
W, H = 1242, 375
XR_G = np.array([[0.96, -0.28, 0.0], [0.28, 0.96, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
XT_G = np.array([0.3, -0.1, 1.65])


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    v = {4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize]
    return np.array_equal(a.view(v), b.view(v))


def _rig_Q(eng):
    """The rig's Q for the default calibration at 1242 x 375, on the host (test_rig.py: sv_rig_matrices returns these bits)."""
    L = eng.lib()
    L.sv_debug_stereo_rectify.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    Q = np.zeros(16)
    yml = os.path.join(os.path.dirname(eng.LIB_PATH), "stereo_vision", "data", "kitti_2011_09_26.yml").encode()
    assert L.sv_debug_stereo_rectify(yml, W, H, 1.0, 1, Q.ctypes.data, None) == 0
    return Q.reshape(4, 4)


# ---------------------------------------------------------------------------------------------------------------- CPU

# 6 x 5 map of powers of two, so that every quotient is exact; -16, 0 and NaN are no candidates, 0.125 quantises to q = 0 (4 d = 0.5
# rounds half to even) but is a candidate of the float form
HAND_D = np.array([[1, 2, -16, 4, 0.5, 1],
                   [0, 0.125, 2, NAN, 1, 8],
                   [1, 1, 0.25, 2, -16, 4],
                   [0.5, 0, 1, 1, 2, 0.125],
                   [2, 4, NAN, 8, 1, 0.5]], np.float32)
HAND_Q = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 8], [0, 0, 1, 0]], np.float64)  # P = (x, y, 8) / d ("d1"), / (4 d) ("dmap")
HAND_XR, HAND_XT = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]), np.array([0.5, -0.25, 2.0])  # P' = (Z + .5, -X - .25, -Y + 2)
OPEN = (None, None)
# (disparity, step, (lo, hi), transform): (index, xyz), worked out by hand, pixel (x, y) has index 6 y + x
HAND = {
    ("d1", 1, OPEN, False): (
        [0, 1, 3, 4, 5, 7, 8, 10, 11, 12, 13, 14, 15, 17, 18, 20, 21, 22, 23, 24, 25, 27, 28, 29],
        [(0, 0, 8), (0.5, 0, 4), (0.75, 0, 2), (8, 0, 16), (5, 0, 8), (8, 8, 64), (1, 0.5, 4), (4, 1, 8), (0.625, 0.125, 1), (0, 2, 8), (1, 2, 8),
         (8, 8, 32), (1.5, 1, 4), (1.25, 0.5, 2), (0, 6, 16), (2, 3, 8), (3, 3, 8), (2, 1.5, 4), (40, 24, 64), (0, 2, 4), (0.25, 1, 2), (0.375, 0.5, 1),
         (4, 4, 8), (10, 8, 16)]),
    ("dmap", 1, OPEN, False): (  # without the two 0.125 pixels (7 and 23)
        [0, 1, 3, 4, 5, 8, 10, 11, 12, 13, 14, 15, 17, 18, 20, 21, 22, 24, 25, 27, 28, 29],
        [(0, 0, 2), (0.125, 0, 1), (0.1875, 0, 0.5), (2, 0, 4), (1.25, 0, 2), (0.25, 0.125, 1), (1, 0.25, 2), (0.15625, 0.03125, 0.25), (0, 0.5, 2),
         (0.25, 0.5, 2), (2, 2, 8), (0.375, 0.25, 1), (0.3125, 0.125, 0.5), (0, 1.5, 4), (0.5, 0.75, 2), (0.75, 0.75, 2), (0.5, 0.375, 1), (0, 0.5, 1),
         (0.0625, 0.25, 0.5), (0.09375, 0.125, 0.25), (1, 1, 2), (2.5, 2, 4)]),
    ("d1", 2, OPEN, False): ([0, 4, 12, 14, 24, 28], [(0, 0, 8), (8, 0, 16), (0, 2, 8), (8, 8, 32), (0, 2, 4), (4, 4, 8)]),  # pixel 2 is -16, 26 NaN
    ("dmap", 2, OPEN, False): ([0, 4, 12, 14, 24, 28], [(0, 0, 2), (2, 0, 4), (0, 0.5, 2), (2, 2, 8), (0, 0.5, 1), (1, 1, 2)]),
    # 0 < X < 4, 0 < Y < 2, 2 < Z < 16: pixel 10 has X = 4, pixel 13 Y = 2, pixel 1 Y = 0, pixel 3 Z = 2, pixel 4 Z = 16 - all on a bound, all out
    ("d1", 1, ((0, 0, 2), (4, 2, 16)), False): ([8, 15, 22], [(1, 0.5, 4), (1.5, 1, 4), (2, 1.5, 4)]),
    # 0 < X < 2, 0 < Y < 2, 0.5 < Z < 4: pixel 14 has X = 2, pixels 17 and 25 Z = 0.5, pixel 4 Z = 4
    ("dmap", 1, ((0, 0, 0.5), (2, 2, 4)), False): (
        [8, 10, 13, 15, 20, 21, 22, 28],
        [(0.25, 0.125, 1), (1, 0.25, 2), (0.25, 0.5, 2), (0.375, 0.25, 1), (0.5, 0.75, 2), (0.75, 0.75, 2), (0.5, 0.375, 1), (1, 1, 2)]),
    ("dmap", 2, ((0, 0, 0.5), (2, 2, 4)), False): ([28], [(1, 1, 2)]),
    ("d1", 1, OPEN, True): (
        [0, 1, 3, 4, 5, 7, 8, 10, 11, 12, 13, 14, 15, 17, 18, 20, 21, 22, 23, 24, 25, 27, 28, 29],
        [(8.5, -0.25, 2), (4.5, -0.75, 2), (2.5, -1, 2), (16.5, -8.25, 2), (8.5, -5.25, 2), (64.5, -8.25, -6), (4.5, -1.25, 1.5), (8.5, -4.25, 1),
         (1.5, -0.875, 1.875), (8.5, -0.25, 0), (8.5, -1.25, 0), (32.5, -8.25, -6), (4.5, -1.75, 1), (2.5, -1.5, 1.5), (16.5, -0.25, -4), (8.5, -2.25, -1),
         (8.5, -3.25, -1), (4.5, -2.25, 0.5), (64.5, -40.25, -22), (4.5, -0.25, 0), (2.5, -0.5, 1), (1.5, -0.625, 1.5), (8.5, -4.25, -2), (16.5, -10.25, -6)]),
    # the crop applies AFTER the transform: the box of the d1 crop above, moved by it (2.5 < X' < 16.5, -4.25 < Y' < -0.25, 0 < Z' < 2)
    ("d1", 1, ((2.5, -4.25, 0), (16.5, -0.25, 2)), True): ([8, 15, 22], [(4.5, -1.25, 1.5), (4.5, -1.75, 1), (4.5, -2.25, 0.5)]),
}


def test_hand_built_map(sv):
    colors = np.arange(5 * 6 * 4, dtype=np.uint8).reshape(5, 6, 4)
    for (kind, step, (lo, hi), xf), (want_index, want_xyz) in HAND.items():
        kw = dict(lo=lo, hi=hi, step=step, disparity=kind, XR=HAND_XR if xf else None, XT=HAND_XT if xf else None)
        for dtype, np_t in (("f32", np.float32), ("f64", np.float64)):
            xyz, color, index = sv.compact_cloud(HAND_D, HAND_Q, dtype=dtype, colors=colors, **kw)
            assert xyz.dtype == np_t and xyz.shape == (len(want_index), 3) and index.dtype == np.int32 and color.dtype == np.uint8, (kind, step, lo)
            assert index.tolist() == want_index, (kind, step, lo, xf, index.tolist())
            assert _bits(xyz, np.array(want_xyz, np_t).reshape(-1, 3)), (kind, step, lo, xf, xyz)
            assert np.array_equal(color, colors.reshape(-1, 4)[want_index])
        assert sv.compact_cloud(HAND_D, HAND_Q, **kw)[1] is None
    # batched input: a list, one tuple per frame, each the frame's own
    out = sv.compact_cloud(np.stack([HAND_D, HAND_D[::-1]]), HAND_Q, disparity="dmap", step=2)
    assert len(out) == 2 and out[0][2].tolist() == HAND[("dmap", 2, OPEN, False)][0] and _bits(out[1][0], sv.compact_cloud(HAND_D[::-1], HAND_Q, disparity="dmap", step=2)[0])
    # a step beyond the image visits pixel (0, 0) alone
    xyz, _, index = sv.compact_cloud(HAND_D, HAND_Q, step=7)
    assert index.tolist() == [0] and xyz.tolist() == [[0, 0, 8]]
    for bad in (dict(step=0), dict(step=1.5), dict(step=True), dict(disparity="depth"), dict(dtype="f16"), dict(lo=(0, 0, 0), hi=(1, 0, 1)),
                dict(lo=(NAN, 0, 0)), dict(hi=(1, 1)), dict(colors=np.zeros((5, 6, 3), np.uint8)), dict(colors=np.zeros((5, 6, 4), np.float32))):
        with pytest.raises(ValueError):
            sv.compact_cloud(HAND_D, HAND_Q, **bad)


def test_restatement_selects_from_the_dense_cloud(sv, eng):
    """compact_cloud on the golden KITTI map == the dense cloud of _reproject_np under a mask written here; the CLI crop in vehicle
    axes, with the rig's Q, keeps a real share and rejects a real share."""
    d = util.golden_npz("kitti0_d256")["final1"].reshape(H, W).astype(np.float32)
    Q = _rig_Q(eng)
    lo, hi = sv.CLI_CLOUD_CROP
    assert (lo, hi) == ((0.0, -20.0, -1.4), (40.0, 20.0, 1.0))
    rng = np.random.default_rng(3)
    colors = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    for kind in ("d1", "dmap"):
        dense = _reproject_np(d[None], Q, sv.CAMERA_TO_VEHICLE, None, quantise=kind == "dmap")[0]
        cand = (np.clip(np.rint(d * np.float32(4.0)), 0, 255) > 0) if kind == "dmap" else d > 0
        for step in (1, 4):
            for crop in (True, False):
                with np.errstate(invalid="ignore"):
                    inside = np.isfinite(dense).all(-1)
                    if crop:
                        inside = (dense[..., 0] > 0) & (dense[..., 0] < 40) & (dense[..., 1] > -20) & (dense[..., 1] < 20) & (dense[..., 2] > -1.4) & (dense[..., 2] < 1.0)
                on_lattice = np.zeros((H, W), bool)
                on_lattice[::step, ::step] = True
                mask = cand & inside & on_lattice
                for dtype in ("f64", "f32"):
                    xyz, color, index = sv.compact_cloud(d, Q, XR=sv.CAMERA_TO_VEHICLE, lo=lo if crop else None, hi=hi if crop else None, step=step,
                                                         disparity=kind, dtype=dtype, colors=colors)
                    want = dense[mask] if dtype == "f64" else dense[mask].astype(np.float32)
                    assert _bits(xyz, want) and np.array_equal(index, np.flatnonzero(mask).astype(np.int32)) and np.array_equal(color, colors[mask])
                if kind == "d1" and crop:
                    kept, rejected = int(mask.sum()), int((cand & on_lattice).sum() - mask.sum())
                    print("d1, CLI crop, step %d: %d kept, %d candidates rejected" % (step, kept, rejected))
                    if step == 1:
                        assert kept >= 10000 and rejected >= 10000, (kept, rejected)
                    else:
                        assert kept >= 500 and rejected >= 500, (kept, rejected)


def _w0_case():
    """A Q whose pos.w vanishes at disparity 2 (Q[3][3] = -2 Q[3][2]) and a map that holds 2.0 and 0.5 (q = 2) among other values."""
    Q = np.array([[1, 0, 0, -3], [0, 1, 0, -2], [0, 0, 0, 8], [0, 0, 1, -2]], np.float64)
    d = np.array([[2, 1, 0.5, 4, 2, -10, 3], [0.5, 2, 8, NAN, 0.5, 2, 1], [1, 0.5, 2, 6, 0, 0.5, 2]], np.float32)
    return d, Q


def test_a_vanishing_w_is_dropped_with_every_axis_open(sv):
    d, Q = _w0_case()
    for kind, zero_at in (("d1", 2.0), ("dmap", 0.5)):
        xyz, _, index = sv.compact_cloud(d, Q, disparity=kind, dtype="f64")
        hit = np.flatnonzero(d.reshape(-1) == zero_at)
        cand = np.flatnonzero(d.reshape(-1) > 0)
        assert len(hit) >= 5 and not set(hit.tolist()) & set(index.tolist()), (kind, index)
        assert sorted(set(cand.tolist()) - set(hit.tolist())) == index.tolist()  # every other candidate is kept
        assert np.isfinite(xyz).all()


def _spec(eng, lo=(-INF,) * 3, hi=(INF,) * 3, disparity=1, step=1, dtype=0, reserved=None):
    sp = eng.SvCloudSpec()
    sp.lo[:], sp.hi[:] = lo, hi
    sp.disparity, sp.step, sp.dtype = disparity, step, dtype
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


def _bad_specs(eng):
    return ([_spec(eng, reserved=k) for k in range(5)] + [_spec(eng, disparity=v) for v in (2, -1)] + [_spec(eng, dtype=v) for v in (2, -1)] +
            [_spec(eng, step=v) for v in (0, -3)] +
            [_spec(eng, lo=lo, hi=hi) for lo, hi in (((0, 0, 0), (1, 0, 1)), ((0, 0, 2), (1, 1, 1)), ((NAN, 0, 0), (1, 1, 1)), ((0, 0, 0), (1, NAN, 1)),
                                                     ((INF, 0, 0), (INF, 1, 1)), ((0, 0, 0), (1, 1, -INF)))])


def _bad_calls(eng, ptr, ws_bytes):
    """(what, return code, text) of every refused call; ptr(name) gives the address of a buffer."""
    L = eng.cloud_lib()
    good = dict(disp=ptr("disp"), colors=ptr("colors"), batch=2, width=16, height=8, Q=ptr("Q"), XR=None, XT=None, spec=_spec(eng), capacity=128,
                xyz=ptr("xyz"), color_out=ptr("color_out"), index_out=ptr("index_out"), counts=ptr("counts"), ws=ptr("ws"), ws_bytes=ws_bytes)

    def call(**kw):
        a = dict(good, **kw)
        sp = ctypes.byref(a["spec"]) if a["spec"] is not None else None
        return L.sv_cloud_disparity_device(a["disp"], a["colors"], a["batch"], a["width"], a["height"], a["Q"], a["XR"], a["XT"], sp, a["capacity"], a["xyz"],
                                           a["color_out"], a["index_out"], a["counts"], a["ws"], a["ws_bytes"], None)

    cases = [dict(spec=None), dict(disp=None), dict(Q=None), dict(counts=None), dict(xyz=None), dict(colors=None), dict(capacity=-1), dict(batch=-1),
             dict(batch=65536), dict(width=0), dict(height=0), dict(width=-5), dict(width=65536, height=32768), dict(width=46341, height=46341),
             dict(ws=None), dict(ws_bytes=7), dict(ws_bytes=0), dict(colors=ptr("colors") + 1), dict(color_out=ptr("color_out") + 2)]
    cases += [dict(spec=sp) for sp in _bad_specs(eng)]
    out = []
    for kw in cases:
        rc = call(**kw)
        out.append((sorted(kw), rc, L.sv_last_error(None)))
    return out, call


def test_validation_needs_no_device(eng):
    """Every SV_ERR_ARG case on host buffers: the checks run before any HIP call, so nothing is read or written; batch == 0 returns
    SV_OK with nothing enqueued.  The workspace size is 4 bytes per tile and pair, SIZE_MAX for bad input."""
    L = eng.cloud_lib()
    for name in ("sv_cloud_disparity_device", "sv_cloud_workspace_bytes", "sv_cloud_tile"):
        assert hasattr(L, name)
    T = eng.cloud_tile()
    assert T >= 64 and T == L.sv_cloud_tile()
    ws = lambda sp, b, w, h: L.sv_cloud_workspace_bytes(ctypes.byref(sp) if sp is not None else None, b, w, h)  # noqa: E731
    assert ws(_spec(eng), 2, 16, 8) == 2 * 4 * -(-128 // T) and ws(_spec(eng), 0, 16, 8) == 0
    assert ws(_spec(eng), 3, 2 * T + 1, 1) == 3 * 4 * 3 and ws(_spec(eng, step=2), 3, 2 * T + 1, 3) == 3 * 4 * -(-(T + 1) * 2 // T)
    assert ws(_spec(eng, step=2 ** 31 - 1), 5, 8192, 4096) == 5 * 4
    assert ws(_spec(eng), 1, 8192, 4096) == 4 * (8192 * 4096 // T)
    for sp in _bad_specs(eng) + [None]:
        assert ws(sp, 2, 16, 8) == SIZE_MAX
    for b, w, h in ((-1, 16, 8), (65536, 16, 8), (2, 0, 8), (2, 16, 0), (2, 65536, 32768), (2, -4, -4)):
        assert ws(_spec(eng), b, w, h) == SIZE_MAX
    bufs = {k: np.full(8192, 0x5A, np.uint8) for k in ("disp", "colors", "xyz", "color_out", "index_out", "counts", "ws")}
    bufs["Q"] = np.eye(4).reshape(16)
    calls, call = _bad_calls(eng, lambda name: bufs[name].ctypes.data, ws(_spec(eng), 2, 16, 8))
    assert len(calls) == 19 + 17
    for what, rc, text in calls:
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_cloud"), (what, rc, text)
    assert call(batch=0) == 0 and call(batch=0, ws=None, ws_bytes=0) == 0
    assert all((bufs[k] == 0x5A).all() for k in bufs if k != "Q")
    for bad in (dict(step=0), dict(step=2 ** 31), dict(step=0.5), dict(disparity="depth"), dict(dtype="f16"), dict(lo=(0, 0, 0), hi=(0, 1, 1)),
                dict(lo=(0, NAN, 0)), dict(hi=(1, 2, 3, 4))):
        with pytest.raises(ValueError):
            eng.cloud_spec(**bad)
    sp = eng.cloud_spec(lo=(0, -20, -1.4), hi=(40, 20, 1.0), step=3, disparity="dmap", dtype="f64")
    assert (list(sp.lo), list(sp.hi), sp.disparity, sp.step, sp.dtype, list(sp.reserved)) == ([0, -20, -1.4], [40, 20, 1.0], 0, 3, 1, [0] * 5)
    assert ctypes.sizeof(sp) == 80 and list(eng.cloud_spec().lo) == [-INF] * 3 and list(eng.cloud_spec().hi) == [INF] * 3


def _read_ply(path):
    with open(path, "rb") as f:
        raw = f.read()
    head, payload = raw.split(b"end_header\n", 1)
    return head.decode("ascii").split("\n")[:-1], payload


def test_write_ply(sv, tmp_path):
    rng = np.random.default_rng(2)
    xyz = rng.uniform(-50, 50, (1000, 3))
    color = rng.integers(0, 256, (1000, 4), dtype=np.uint8)
    sv.write_ply(tmp_path / "c.ply", xyz, color)
    head, payload = _read_ply(tmp_path / "c.ply")
    assert head == ["ply", "format binary_little_endian 1.0", "element vertex 1000", "property float x", "property float y", "property float z",
                    "property uchar red", "property uchar green", "property uchar blue"]
    rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
    assert rec.shape == (1000,) and len(payload) == 1000 * 15
    assert _bits(rec["xyz"], xyz.astype(np.float32)) and np.array_equal(rec["rgb"], color[:, 2::-1])  # BGRA -> red green blue
    sv.write_ply(tmp_path / "p.ply", xyz.astype(np.float32)[:7])
    head, payload = _read_ply(tmp_path / "p.ply")
    assert head[2] == "element vertex 7" and len(head) == 6 and _bits(np.frombuffer(payload, "<f4").reshape(7, 3), xyz.astype(np.float32)[:7])
    sv.write_ply(tmp_path / "e.ply", np.zeros((0, 3), np.float32), np.zeros((0, 4), np.uint8))
    head, payload = _read_ply(tmp_path / "e.ply")
    assert head[2] == "element vertex 0" and payload == b""
    for bad in ((xyz[:, :2], None), (xyz, color[:, :3]), (xyz, color[:10]), (xyz, color.astype(np.int32))):
        with pytest.raises(ValueError):
            sv.write_ply(tmp_path / "bad.ply", *bad)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _gpu(eng, d, Q, colors=None, **kw):
    """The engine call on numpy inputs -> (per-frame [(xyz, color or None, index)], counts) as numpy."""
    d = np.asarray(d, np.float32)
    d = d[None] if d.ndim == 2 else d
    if colors is not None:
        colors = _cuda(colors[None] if colors.ndim == 3 else colors)
    xyz, color, index, counts = eng.compact_cloud_from_disparity(_cuda(d), Q, colors=colors, want_index=True, **kw)
    assert xyz.is_cuda and counts.is_cuda and counts.dtype.is_floating_point is False and tuple(counts.shape) == (d.shape[0],)
    frames = [tuple(None if t is None else t.cpu().numpy() for t in f) for f in eng.split_clouds(xyz, counts, color, index)]
    return frames, counts.cpu().numpy()


def _check(sv, eng, d, Q, colors=None, want=None, **kw):
    """GPU == restatement for every frame of d; returns the counts."""
    d = np.asarray(d, np.float32)
    d = d[None] if d.ndim == 2 else d
    got, counts = _gpu(eng, d, Q, colors, **kw)
    if want is None:
        want = sv.compact_cloud(d, Q, colors=colors if colors is None or colors.ndim == 4 else colors[None],
                                **{k: v for k, v in kw.items() if k != "capacity"})
    assert len(got) == len(want) == d.shape[0]
    cap = kw.get("capacity")
    for b, ((gx, gc, gi), (wx, wc, wi)) in enumerate(zip(got, want)):
        n = len(wi) if cap is None else min(len(wi), cap)
        assert counts[b] == len(wi), (b, counts[b], len(wi), kw)
        assert np.array_equal(gi, wi[:n]), (b, kw)
        assert _bits(gx, wx[:n]), (b, kw)
        assert (gc is None) == (wc is None) and (gc is None or np.array_equal(gc, wc[:n])), (b, kw)
        assert not np.isnan(gx).any()
    return counts


CROPS = {"open": (None, None), "cli": ((0.0, -20.0, -1.4), (40.0, 20.0, 1.0)), "half_open": ((-INF, -1.5, 2.0), (INF, INF, 30.0))}
XFS = {"none": (None, None), "vehicle": (np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]]), None), "general": (XR_G, XT_G)}


@functools.lru_cache(maxsize=None)
def _kitti_colors():
    return np.random.default_rng(17).integers(0, 256, (3, H, W, 4), dtype=np.uint8)


_restated = {}


def _kitti_restated(sv, d1, Q, kind, step, crop, xf):
    """The f64 restatement with colours of the three KITTI frames, once per (disparity, step, crop, transform)."""
    key = (kind, step, crop, xf)
    if key not in _restated:
        (lo, hi), (XR, XT) = CROPS[crop], XFS[xf]
        _restated[key] = sv.compact_cloud(d1, Q, XR=XR, XT=XT, lo=lo, hi=hi, step=step, disparity=kind, dtype="f64", colors=_kitti_colors())
    return _restated[key]


@pytest.mark.gpu
@pytest.mark.parametrize("with_colors", [True, False])
@pytest.mark.parametrize("xf", list(XFS))
@pytest.mark.parametrize("crop", list(CROPS))
@pytest.mark.parametrize("step", [1, 2, 3, 7])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["dmap", "d1"])
def test_fused_equals_restatement(sv, eng, kitti_d1, kind, dtype, step, crop, xf, with_colors):
    d1, Q = kitti_d1
    (lo, hi), (XR, XT) = CROPS[crop], XFS[xf]
    want = _kitti_restated(sv, d1, Q, kind, step, crop, xf)
    if dtype == "f32":  # the restatement's float32 form is astype(float32) of these doubles (checked against compact_cloud itself below)
        with np.errstate(over="ignore"):
            want = [(x.astype(np.float32), c, i) for x, c, i in want]
        if (step, crop, xf, with_colors) == (3, "cli", "vehicle", True):
            direct = sv.compact_cloud(d1, Q, XR=XR, XT=XT, lo=lo, hi=hi, step=step, disparity=kind, dtype="f32")
            assert all(_bits(a[0], b[0]) for a, b in zip(direct, want))
    if not with_colors:
        want = [(x, None, i) for x, _, i in want]
    counts = _check(sv, eng, d1, Q, _kitti_colors() if with_colors else None, want=want, XR=XR, XT=XT, lo=lo, hi=hi, step=step, disparity=kind, dtype=dtype)
    if (kind, step, crop, xf) == ("d1", 1, "cli", "vehicle"):  # the product case keeps a real share and rejects a real share
        assert counts[0] >= 10000 and (d1[0] > 0).sum() - counts[0] >= 10000, counts
    if crop == "open" and kind == "d1":
        assert counts[0] == (d1[0, ::step, ::step] > 0).sum()  # the rig's Q has no positive disparity with pos.w = 0


def _random_map(rng, h, w, density):
    d = rng.uniform(0.3, 80.0, (h, w)).astype(np.float32)
    bad = rng.random((h, w)) >= density
    d[bad] = rng.choice(np.array([NAN, -10.0, 0.0, INF], np.float32), int(bad.sum()))  # +inf: q = 255 ("dmap"), a candidate of "d1" too
    return d


SMALL_Q = np.array([[1, 0, 0, -30.5], [0, 1, 0, -17.25], [0, 0, 0, 700.0], [0, 0, 1 / 0.54, 0]], np.float64)


@pytest.mark.gpu
def test_shapes_around_the_tiling(sv, eng):
    T = eng.cloud_tile()
    rng = np.random.default_rng(23)
    shapes = [(1, 1), (1, 70), (70, 1), (5, 63), (5, 64), (5, 65), (3, 1241), (1, T - 1), (1, T), (1, T + 1), (1, 4 * T - 1), (1, 4 * T), (1, 4 * T + 1),
              (7, 4 * T + 3)]
    for h, w in shapes:
        d = _random_map(rng, h, w, 0.7)
        colors = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        for kind, dtype in (("d1", "f32"), ("dmap", "f64")):
            _check(sv, eng, d, SMALL_Q, colors, disparity=kind, dtype=dtype)
        _check(sv, eng, d, SMALL_Q, colors, step=2, lo=(-INF, -INF, 10.0), hi=(INF, INF, 400.0))
    # the visited lattice, not the image, is what is tiled: step 3 over 3 T - 2 columns visits T of them
    for n in (T - 1, T, T + 1):
        d = _random_map(rng, 4, 3 * n - 2, 0.6)
        assert d[::3, ::3].shape == (2, n)
        _check(sv, eng, d, SMALL_Q, step=3)
    # a step beyond the image: pixel (0, 0) alone is visited
    d = _random_map(rng, 40, 50, 1.0)
    for step in (50, 51, 1000, 2 ** 31 - 1):
        counts = _check(sv, eng, d, SMALL_Q, step=step, dtype="f64")
        assert counts.tolist() == [1]
    # frames whose rows do not start on 16 bytes (odd width, second frame): the scalar loads of the same layout
    _check(sv, eng, np.stack([_random_map(rng, 9, 333, 0.5) for _ in range(4)]), SMALL_Q)


@pytest.mark.gpu
def test_a_4k_frame(sv, eng):
    rng = np.random.default_rng(29)
    d = _random_map(rng, 2160, 3840, 0.8)
    Q = np.array([[1, 0, 0, -1920.0], [0, 1, 0, -1080.0], [0, 0, 0, 2800.0], [0, 0, 1 / 0.3, 0]], np.float64)
    colors = rng.integers(0, 256, (2160, 3840, 4), dtype=np.uint8)
    counts = _check(sv, eng, d, Q, colors, lo=(-40, -20, 0.5), hi=(40, 20, 60.0))
    assert 100000 < counts[0] < 0.8 * d.size


@pytest.mark.gpu
def test_contents(sv, eng):
    rng = np.random.default_rng(31)
    h, w = 61, 517
    colors = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    invalid = rng.choice(np.array([NAN, -10.0, 0.0, -0.0, -INF], np.float32), (h, w))
    valid = rng.uniform(1.0, 60.0, (h, w)).astype(np.float32)
    last = invalid.copy()
    last[-1, -1] = 7.5
    for kind in ("d1", "dmap"):
        assert _check(sv, eng, invalid, SMALL_Q, colors, disparity=kind).tolist() == [0]
        assert _check(sv, eng, valid, SMALL_Q, colors, disparity=kind).tolist() == [h * w]
        assert _check(sv, eng, last, SMALL_Q, colors, disparity=kind).tolist() == [1]
        for density in (0.01, 0.5, 0.99):
            _check(sv, eng, _random_map(rng, h, w, density), SMALL_Q, colors, disparity=kind, dtype="f64")
    # +inf: d > 0, so a candidate of the float form - but a row of Q either has a 0 beside the disparity (0 * inf = NaN) or makes the
    # row infinite (inf / inf = NaN), so no Q gives it a point and the strict comparison drops it; the 8-bit form saturates it to q = 255
    infinite = np.full((h, w), INF, np.float32)
    dense_q = np.array([[1, 0, 2, 0], [0, 1, 3, 0], [0, 0, 5, 8], [0, 0, 1, 0]], np.float64)  # no 0 beside the disparity in any row
    for Q in (SMALL_Q, HAND_Q, dense_q):
        assert _check(sv, eng, infinite, Q, colors, disparity="d1").tolist() == [0]
        assert _check(sv, eng, infinite, Q, colors, disparity="dmap").tolist() == [h * w]
    mixed = np.where(rng.random((h, w)) < 0.3, np.float32(INF), valid)
    for kind in ("d1", "dmap"):
        for Q in (SMALL_Q, dense_q):
            counts = _check(sv, eng, mixed, Q, colors, disparity=kind, dtype="f64")
            assert counts[0] == (np.isfinite(mixed).sum() if kind == "d1" else h * w)
    # nothing is written for an all-invalid frame
    import torch
    xyz = torch.full((1, h * w, 3), -7.25, dtype=torch.float32, device="cuda")
    counts = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    _raw(eng, _cuda(invalid[None]), None, SMALL_Q, eng.cloud_spec(), h * w, xyz, None, None, counts)
    torch.cuda.synchronize()
    assert counts.item() == 0 and (xyz == -7.25).all().item()
    # pos.w = 0 for one positive disparity: candidates, yet dropped, with every axis open
    d, Q = _w0_case()
    big = np.tile(d, (20, 30))
    for kind, zero_at in (("d1", 2.0), ("dmap", 0.5)):
        counts = _check(sv, eng, big, Q, disparity=kind, dtype="f64")
        assert counts[0] == ((big > 0) & (big != zero_at)).sum() < (big > 0).sum()
    # a coordinate beyond the float range passes the crop in double and becomes inf in float32
    Qf = np.array([[1e300, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 8], [0, 0, 1, 0]], np.float64)
    (frames, counts) = _gpu(eng, valid, Qf)
    assert counts[0] == h * w and np.isinf(frames[0][0][:, 0]).sum() == h * (w - 1)
    _check(sv, eng, valid, Qf)


def _raw(eng, d_t, colors_t, Q, spec, capacity, xyz, color, index, counts, XR=None, XT=None, stream=None):
    """The C entry on caller-owned buffers (torch tensors), the workspace from torch."""
    import torch
    L = eng.cloud_lib()
    B, Hh, Ww = d_t.shape
    n = L.sv_cloud_workspace_bytes(ctypes.byref(spec), B, Ww, Hh)
    assert n != SIZE_MAX
    ws = torch.empty((max(n // 4, 1),), dtype=torch.int32, device="cuda")
    q = np.ascontiguousarray(Q, np.float64).reshape(16)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = L.sv_cloud_disparity_device(d_t.data_ptr(), ptr(colors_t), B, Ww, Hh, q.ctypes.data, None if XR is None else XR.ctypes.data,
                                     None if XT is None else XT.ctypes.data, ctypes.byref(spec), capacity, ptr(xyz), ptr(color), ptr(index), counts.data_ptr(),
                                     ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream if stream is None else stream)
    assert rc == 0, (rc, L.sv_last_error(None))
    return ws


@pytest.mark.gpu
def test_capacity(sv, eng, kitti_d1):
    import torch
    d1, Q = kitti_d1
    colors = _kitti_colors()
    kw = dict(lo=CROPS["cli"][0], hi=CROPS["cli"][1], XR=XFS["vehicle"][0])
    want = sv.compact_cloud(d1, Q, colors=colors, **kw)
    full = np.array([len(w[2]) for w in want])
    assert full.min() > 5000
    t, c = _cuda(d1), _cuda(colors)
    spec = eng.cloud_spec(lo=kw["lo"], hi=kw["hi"])
    for cap in (1, 1000, 4097, int(full.min()), int(full.max()) + 5):
        _check(sv, eng, d1, Q, colors, want=want, capacity=cap, **kw)
        # rows beyond min(count, capacity) stay as they were: poisoned buffers with a guard row block behind every frame's slot
        xyz = torch.full((3, cap, 3), -7.25, dtype=torch.float32, device="cuda")
        col = torch.full((3, cap, 4), 0x5A, dtype=torch.uint8, device="cuda")
        idx = torch.full((3, cap), -77, dtype=torch.int32, device="cuda")
        counts = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        _raw(eng, t, c, Q, spec, cap, xyz, col, idx, counts, XR=np.ascontiguousarray(kw["XR"]))
        torch.cuda.synchronize()
        assert np.array_equal(counts.cpu().numpy(), full)
        for b in range(3):
            n = min(int(full[b]), cap)
            assert _bits(xyz[b, :n].cpu().numpy(), want[b][0][:n]) and np.array_equal(idx[b, :n].cpu().numpy(), want[b][2][:n])
            assert np.array_equal(col[b, :n].cpu().numpy(), want[b][1][:n])
            assert (xyz[b, n:] == -7.25).all().item() and (col[b, n:] == 0x5A).all().item() and (idx[b, n:] == -77).all().item()
    # capacity 0: counts only, nothing else is touched (xyz may be NULL)
    counts = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    _raw(eng, t, c, Q, spec, 0, None, None, None, counts, XR=np.ascontiguousarray(kw["XR"]))
    torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy(), full)
    xyz, col, idx, counts = eng.compact_cloud_from_disparity(t, Q, colors=c, capacity=0, want_index=True, **kw)
    assert tuple(xyz.shape) == (3, 0, 3) and tuple(col.shape) == (3, 0, 4) and tuple(idx.shape) == (3, 0) and np.array_equal(counts.cpu().numpy(), full)
    assert all(f[0].shape[0] == 0 for f in eng.split_clouds(xyz, counts, col))
    for bad in (-1, 1.5, 2 ** 31):
        with pytest.raises(ValueError):
            eng.compact_cloud_from_disparity(t, Q, capacity=bad)


@pytest.mark.gpu
def test_batches_and_repeats(sv, eng, kitti_d1):
    import torch
    d1, Q = kitti_d1
    rng = np.random.default_rng(37)
    frames = np.stack([d1[0], d1[1], d1[2], _random_map(rng, H, W, 0.3), np.where(d1[0] > 20, d1[0], np.float32(-10))])
    colors = rng.integers(0, 256, (5, H, W, 4), dtype=np.uint8)
    kw = dict(XR=XR_G, XT=XT_G, lo=(-5, -30, -2), hi=(60, 30, 4), step=2)
    batch, counts = _gpu(eng, frames, Q, colors, **kw)
    assert len(set(counts.tolist())) == 5 and counts.min() > 0
    for b in range(5):
        alone, n = _gpu(eng, frames[b], Q, colors[b], **kw)
        assert n[0] == counts[b] and all(_bits(x, y) for x, y in zip(alone[0], batch[b]))
    again, counts2 = _gpu(eng, frames, Q, colors, **kw)
    assert np.array_equal(counts, counts2) and all(_bits(x, y) for f, g in zip(batch, again) for x, y in zip(f, g))
    # an empty batch: nothing is enqueued, empty outputs
    xyz, col, idx, n = eng.compact_cloud_from_disparity(torch.empty((0, 8, 16), device="cuda"), Q, want_index=True)
    assert tuple(xyz.shape) == (0, 128, 3) and col is None and tuple(idx.shape) == (0, 128) and tuple(n.shape) == (0,) and eng.split_clouds(xyz, n) == []
    guard = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    L = eng.cloud_lib()
    sp = eng.cloud_spec()
    assert L.sv_cloud_disparity_device(guard.data_ptr(), None, 0, 16, 8, np.eye(4).ctypes.data, None, None, ctypes.byref(sp), 4, guard.data_ptr(), None, None,
                                       guard.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert (guard == -1).all().item()
    # 300 small frames
    small = np.stack([_random_map(rng, 23, 41, 0.6) for _ in range(300)])
    counts = _check(sv, eng, small, SMALL_Q, rng.integers(0, 256, (300, 23, 41, 4), dtype=np.uint8), dtype="f64")
    assert len(set(counts.tolist())) > 20
    # colours that start at an odd storage offset (the C entry refuses them: a pixel moves as one dword) are copied by the engine layer
    flat = torch.zeros(3 * H * W * 4 + 3, dtype=torch.uint8, device="cuda")
    odd = flat[3:].view(3, H, W, 4)
    odd.copy_(_cuda(colors[:3]))
    assert odd.data_ptr() % 4 == 3 and odd.is_contiguous()
    a = eng.compact_cloud_from_disparity(_cuda(d1), Q, colors=odd, step=3)
    b = eng.compact_cloud_from_disparity(_cuda(d1), Q, colors=_cuda(colors[:3]), step=3)
    assert torch.equal(a[3], b[3]) and all(torch.equal(x[1], y[1]) for x, y in zip(eng.split_clouds(a[0], a[3], a[1]), eng.split_clouds(b[0], b[3], b[1])))
    # input checks of the engine layer
    t = _cuda(d1)
    for bad in (dict(d1=t.double()), dict(d1=t.cpu()), dict(colors=_cuda(colors[:3, :, :, :3])), dict(colors=_cuda(colors[:2])), dict(colors=colors[:3]),
                dict(step=0), dict(disparity="depth"), dict(dtype="f16"), dict(lo=(0, 0, 0), hi=(1, 1, 0))):
        with pytest.raises(ValueError):
            eng.compact_cloud_from_disparity(**dict(dict(d1=t, Q=Q), **bad))


@pytest.mark.gpu
def test_on_torch_current_stream(eng, kitti_d1):
    """Inputs written by torch ops on a busy side stream and a dependent torch op behind the call, no explicit synchronisation in
    between: the results are those of the inputs at rest."""
    import torch
    d1, Q = kitti_d1
    colors = _kitti_colors()
    kw = dict(XR=XFS["vehicle"][0], lo=CROPS["cli"][0], hi=CROPS["cli"][1], want_index=True)
    want = [t.cpu().numpy() for t in eng.compact_cloud_from_disparity(_cuda(d1), Q, colors=_cuda(colors), **kw)]
    src_d, src_c = _cuda(d1), _cuda(colors)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):
            x = x @ x  # keeps the stream busy while the host runs ahead
        d = torch.zeros_like(src_d)
        d.copy_(src_d)
        c = torch.zeros_like(src_c)
        c.copy_(src_c)
        xyz, col, idx, counts = eng.compact_cloud_from_disparity(d, Q, colors=c, **kw)
        total = counts.sum()  # dependent ops on the same stream
        first = torch.stack([xyz[b, 0] for b in range(3)]) * 2
    torch.cuda.synchronize()
    del x
    n = want[3]
    assert np.array_equal(counts.cpu().numpy(), n) and total.item() == n.sum()
    for b in range(3):
        for got, ref in zip((xyz, col, idx), want[:3]):
            assert _bits(got[b, :n[b]].cpu().numpy(), ref[b, :n[b]])
    assert _bits(first.cpu().numpy(), np.stack([want[0][b, 0] for b in range(3)]) * 2)


@pytest.mark.gpu
def test_fused_equals_unfused(eng, kitti_d1):
    """The fused output == torch's mask-and-gather over sv_reproject_batch_device's dense cloud ("dmap", float64), bit for bit."""
    import torch
    d1, Q = kitti_d1
    t = _cuda(d1)
    for XR, XT in ((None, None), (XR_G, XT_G)):
        dmap, cloud = eng.reproject(t, Q, XR, XT)
        xyz, _, idx, counts = eng.compact_cloud_from_disparity(t, Q, XR=XR, XT=XT, disparity="dmap", dtype="f64", want_index=True)
        mask = (dmap > 0) & torch.isfinite(cloud).all(-1)
        for b, (p, i) in enumerate(eng.split_clouds(xyz, counts, idx)):
            ref = cloud[b][mask[b]]
            assert p.shape == ref.shape and torch.equal(p.view(torch.int64), ref.view(torch.int64))
            assert torch.equal(i.long(), torch.nonzero(mask[b].reshape(-1)).reshape(-1))
        assert counts.min().item() > 100000


def _colour_pairs(n=2, seed=11):
    rng = np.random.default_rng(seed)
    ls, rs = [util.load_png("kitti0_color_left.png")], [util.load_png("kitti0_color_right.png")]
    for k in range(1, n):
        off = rng.integers(-40, 40, 3)
        for side, dst in (("left", ls), ("right", rs)):
            dst.append(np.clip(util.load_png("kitti%d_%s.png" % (k, side)).astype(np.int64)[..., None] + off, 0, 255).astype(np.uint8))
    return np.ascontiguousarray(np.stack(ls)[..., ::-1]), np.ascontiguousarray(np.stack(rs)[..., ::-1])  # BGR


@pytest.mark.gpu
def test_rig_compact_clouds(sv, eng, tmp_path):
    import torch
    rigmod, engmod = util.pkg("rig"), util.pkg("engine")
    bgr_l, bgr_r = _colour_pairs()
    kw = dict(lo=CROPS["cli"][0], hi=CROPS["cli"][1], transform=(sv.CAMERA_TO_VEHICLE, None))
    rig = rigmod.StereoRig(W, H)
    try:
        tl, tr = _cuda(bgr_l), _cuda(bgr_r)
        xyz, color, counts = rig.compact_clouds(tl, tr, **kw)
        d1 = rig.disparity(tl, tr)
        col = rig.frontend(tl, tr, colors=True)[2]
        ref = eng.compact_cloud_from_disparity(d1, rig.Q, colors=col, XR=sv.CAMERA_TO_VEHICLE, lo=kw["lo"], hi=kw["hi"])
        assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (xyz, color, counts)) and tuple(xyz.shape) == (2, W * H, 3) and xyz.dtype == torch.float32
        n = counts.cpu().numpy()
        assert np.array_equal(n, ref[3].cpu().numpy()) and n.min() > 10000
        for b in range(2):
            assert torch.equal(xyz[b, :n[b]].view(torch.int32), ref[0][b, :n[b]].view(torch.int32)) and torch.equal(color[b, :n[b]], ref[1][b, :n[b]])
        # the restatement on the same maps and colours
        want = sv.compact_cloud(d1.cpu().numpy(), rig.Q, XR=sv.CAMERA_TO_VEHICLE, lo=kw["lo"], hi=kw["hi"], colors=col.cpu().numpy())
        # numpy in: per-frame numpy arrays
        frames = rig.compact_clouds(bgr_l, bgr_r, **kw)
        assert isinstance(frames, list) and len(frames) == 2
        for b, (p, c) in enumerate(frames):
            assert isinstance(p, np.ndarray) and isinstance(c, np.ndarray) and p.shape == (n[b], 3) and c.shape == (n[b], 4)
            assert _bits(p, want[b][0]) and np.array_equal(c, want[b][1]) and _bits(p, xyz[b, :n[b]].cpu().numpy())
        # other options: no colours, f64, dmap, step, capacity
        p2, c2, n2 = rig.compact_clouds(tl, tr, colors=False, dtype="f64", disparity="dmap", step=3, capacity=5000)
        assert c2 is None and tuple(p2.shape) == (2, 5000, 3) and p2.dtype == torch.float64
        want2 = sv.compact_cloud(d1.cpu().numpy(), rig.Q, dtype="f64", disparity="dmap", step=3)
        for b in range(2):
            assert n2[b].item() == len(want2[b][2]) > 5000 and _bits(p2[b].cpu().numpy(), want2[b][0][:5000])
        assert rig.compact_clouds(bgr_l, bgr_r, colors=False, step=5)[0][1] is None
        for bad in (dict(step=0), dict(disparity="depth"), dict(dtype="f16"), dict(lo=(0, 0, 0), hi=(0, 1, 1)), dict(transform="sideways")):
            with pytest.raises(ValueError):
                rig.compact_clouds(bgr_l, bgr_r, **bad)
        # transform="rig": the default calibration file carries XR / XT, and they are what is applied
        assert rig.XR is not None and rig.XT is not None
        by_name, by_value = rig.compact_clouds(bgr_l, bgr_r, transform="rig", dtype="f64"), rig.compact_clouds(bgr_l, bgr_r, transform=(rig.XR, rig.XT), dtype="f64")
        assert all(_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(by_name, by_value)) and len(by_name[0][0]) > 100000
    finally:
        rig.close()
    # a calibration file without XR / XT: transform="rig" has nothing to apply and raises
    with open(os.path.join(os.path.dirname(eng.LIB_PATH), "stereo_vision", "data", "kitti_2011_09_26.yml")) as f:
        text = f.read()
    assert "\nXR:" in text and text.index("\nXR:") < text.index("\nXT:")
    with open(tmp_path / "no_transform.yml", "w") as f:
        f.write(text[:text.index("\nXR:") + 1])
    bare = rigmod.StereoRig(W, H, calibration=str(tmp_path / "no_transform.yml"))
    try:
        assert bare.XR is None and bare.XT is None
        with pytest.raises(ValueError):
            bare.compact_clouds(bgr_l, bgr_r, transform="rig")
        with pytest.raises(ValueError):
            bare.compact_clouds(_cuda(bgr_l), _cuda(bgr_r), transform="rig", colors=False)
        assert len(bare.compact_clouds(bgr_l, bgr_r)) == 2  # the rig itself works
    finally:
        bare.close()
    p = engmod.SvParams.driver(255)
    p.subsampling = 1
    half = rigmod.StereoRig(W, H, params=p)
    try:
        with pytest.raises(ValueError):
            half.compact_clouds(bgr_l, bgr_r)
    finally:
        half.close()


@pytest.mark.gpu
def test_cli_ply_writes_rig_clouds(sv, tmp_path):
    from PIL import Image
    for d in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / d)
    bgr_l, bgr_r = _colour_pairs(3, seed=3)
    for i in range(3):
        Image.fromarray(bgr_l[i][..., ::-1]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(bgr_r[i][..., ::-1]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with pytest.raises(SystemExit):
        sv.main(["-k", str(tmp_path / "kitti"), "--ply", str(tmp_path / "ply")])  # needs --batch
    sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply")])
    rig = util.pkg("rig").StereoRig(W, H)
    try:
        want = rig.compact_clouds(bgr_l, bgr_r, lo=sv.CLI_CLOUD_CROP[0], hi=sv.CLI_CLOUD_CROP[1], transform=(sv.CAMERA_TO_VEHICLE, None))
    finally:
        rig.close()
    for i, (xyz, color) in enumerate(want):
        head, payload = _read_ply(tmp_path / "ply" / ("%010d.ply" % i))
        rec = np.frombuffer(payload, dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]))
        assert head[2] == "element vertex %d" % len(xyz) and len(xyz) > 10000
        assert _bits(rec["xyz"], xyz) and np.array_equal(rec["rgb"], color[:, 2::-1])
