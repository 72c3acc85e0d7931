"""Ground plane, obstacle labels and free space (include/stereo_vision_hip.h (G)): the numpy definition in stereo_vision.sv on a
hand-built map and on synthetic scenes with a known ground, ground_pose against its closed form, the C ABI's argument checks, and the
HIP kernels - C entry, engine and rig layers - against the definition.

Everything is compared exactly.  That is derived, not chosen: the only floating-point operations between a disparity and any of the
five outputs are 4.0f * d (exact: a power of two) and the rounding of that product to an integer (round half to even on both sides);
the rest is integer counting, integer division and comparison."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import util
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)

SV_ERR_ARG = -1
SIZE_MAX = 2 ** 64 - 1
NAN, INF = float("nan"), float("inf")
W, H, D = 1242, 375, 128
TRUTH = (168, 178)  # the fit of the noisy truth field of synth.disparity_field at 375 x 1242, D = 128 (vh = 168.75, qb = 178.3)
OUTPUTS = ("vdisp", "ground", "labels", "free_row", "free_disp")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype.itemsize != b.dtype.itemsize:
        return False
    v = {4: np.int32, 8: np.int64, 1: np.uint8}[a.dtype.itemsize]
    return np.array_equal(a.view(v), b.view(v))


# ---------------------------------------------------------------------------------------------------------------- CPU

# 6 rows x 8 columns, 16 bins.  The ground is d = v / 2 (bins 0, 2, 4, 6, 8, 10 on rows 0 .. 5: horizon row 0, bin 10 at the bottom);
# column 3 carries an obstacle of two rows, column 6 one of four rows above a ground pixel, column 7 one of five; (4, 2) is a hole
# below the ground.  0.125, 0.375 and 0.625 are the ties of the rounding: 4 d = 0.5, 1.5, 2.5 -> 0, 2, 2.  100 saturates to bin 15.
HAND_D = np.array([[-10, 0.125, 0.125, NAN, 0, 0.25, 3, 100],
                   [0.5, 0.5, 0.5, 0.5, 0.375, 0.625, 3, 2.5],
                   [1, 1, 1, 1, -10, 1, 3, 2.5],
                   [1.5, 1.5, 1.5, 2.5, 1.5, 1.5, 3, 2.5],
                   [2, 2, 0.5, 2.5, 2, 2, 2, 2.5],
                   [2.5, 2.5, 2.5, 2.5, 2.5, -10, 2.5, 2.5]], np.float32)
HAND_VDISP = {0: {0: 2, 1: 1, 12: 1, 15: 1}, 1: {2: 6, 10: 1, 12: 1}, 2: {4: 5, 10: 1, 12: 1}, 3: {6: 5, 10: 2, 12: 1}, 4: {2: 1, 8: 5, 10: 2}, 5: {10: 7}}
HAND_GROUND = [0, 10, 6 + 5 + 5 + 5 + 7, 43]  # rows 1 .. 5 of the line's own bins; 5 + 8 + 7 + 8 + 8 + 7 valid pixels
HAND_LABELS = np.array([[0, 1, 1, 0, 0, 1, 2, 2],  # g_tol = 1, row 0 is the horizon row: g = 0
                        [1, 1, 1, 1, 1, 1, 2, 2],
                        [1, 1, 1, 1, 0, 1, 2, 2],
                        [1, 1, 1, 2, 1, 1, 2, 2],
                        [1, 1, 3, 2, 1, 1, 1, 2],
                        [1, 1, 1, 1, 1, 0, 1, 1]], np.uint8)
HAND_FREE = {1: ([-1, -1, -1, 4, -1, -1, 3, 4], [0, 0, 0, 2.5, 0, 0, 3, 2.5]), 2: ([-1, -1, -1, 4, -1, -1, 3, 4], [0, 0, 0, 2.5, 0, 0, 3, 2.5]),
             3: ([-1, -1, -1, -1, -1, -1, 3, 4], [0, 0, 0, 0, 0, 0, 3, 2.5]), 5: ([-1] * 7 + [4], [0] * 7 + [2.5]), 6: ([-1] * 8, [0] * 8)}
HAND_SPEC = dict(n_bins=16, vh_lo=-2, vh_hi=4, vh_step=1, qb_step=1, tol=0, g_tol=1, min_support=8)


def test_hand_built_map(sv):
    want_vdisp = np.zeros((6, 16), np.uint32)
    for v, bins in HAND_VDISP.items():
        for q, n in bins.items():
            want_vdisp[v, q] = n
    vdisp = sv.v_disparity(HAND_D, 16)
    assert vdisp.dtype == np.uint32 and np.array_equal(vdisp, want_vdisp)
    assert list(sv.ground_line(vdisp, -2, 4, 1, 1, 0, 8)) == HAND_GROUND
    assert sv.ground_row_bins(0, 10, 6).tolist() == [0, 2, 4, 6, 8, 10]
    labels = sv.ground_labels(HAND_D, 16, 0, 10, 1)
    assert labels.dtype == np.uint8 and np.array_equal(labels, HAND_LABELS)
    for min_run, (rows, disps) in HAND_FREE.items():
        fr, fd = sv.free_space(labels, HAND_D, min_run)
        assert fr.dtype == np.int32 and fd.dtype == np.float32 and fr.tolist() == rows and fd.tolist() == disps, min_run
        got = sv.ground(HAND_D, min_run=min_run, **HAND_SPEC)
        assert got["ground"].tolist() == HAND_GROUND and np.array_equal(got["labels"], HAND_LABELS) and got["free_row"].tolist() == rows
    # a support the line does not reach: no ground, every valid pixel below it, no free-space row; S and n_valid stay
    none = sv.ground(HAND_D, min_run=1, **dict(HAND_SPEC, min_support=29))
    assert none["ground"].tolist() == [-1, -1, 28, 43] and np.array_equal(none["labels"], np.where(HAND_D > 0, 3, 0)) and none["free_row"].tolist() == [-1] * 8
    # a wider ground band swallows the hole and the obstacles of column 3 and 7 (e = 2 .. 4) but not column 6's upper rows (e = 6, 8)
    assert np.array_equal(sv.ground_labels(HAND_D, 16, 0, 10, 6)[:, 6], [2, 2, 2, 1, 1, 1])
    # ties of the search: two equal rows of mass - the smallest vh, then the smallest qb
    flat = np.zeros((4, 8), np.uint32)
    flat[3, 2] = flat[3, 3] = 5
    assert list(sv.ground_line(flat, -3, 2, 1, 1, 0, 0)) == [-3, 2, 5, 10]
    assert list(sv.ground_line(flat, 1, 2, 1, 1, 1, 0)) == [1, 2, 10, 10]  # tol 1 around bin 1 reaches bin 2 alone, around bins 2 and 3 both
    assert list(sv.ground_line(flat, 1, 2, 1, 3, 0, 0)) == [1, 3, 5, 10]   # qb = 3, 6
    for bad in (dict(n_bins=7), dict(n_bins=4097), dict(vh_lo=-32769), dict(vh_lo=3, vh_hi=2), dict(vh_hi=5), dict(vh_step=0), dict(qb_step=0), dict(qb_step=16),
                dict(tol=-1), dict(tol=17), dict(g_tol=-1), dict(g_tol=4097), dict(min_run=0), dict(min_support=-1), dict(tol=1.5), dict(min_run=True)):
        with pytest.raises(ValueError):
            sv.ground(HAND_D, **dict(HAND_SPEC, **bad))


def _noisy_truth(seed):
    """(map, mask of the true ground's pixels): the truth field of synth.make_pair(seed) - the texture is drawn first, so that the
    generator's state is the pair's - plus N(0, 0.3) noise, 10 % of the pixels invalid."""
    synth = util.pkg("synth")
    rng = np.random.default_rng(seed)
    rng.integers(0, 256, (H, W + D), dtype=np.uint8)
    field = synth.disparity_field(rng, H, W, D)
    noise = np.random.default_rng(seed + 7)
    d = (field + noise.normal(0, 0.3, (H, W))).astype(np.float32)
    d[noise.random((H, W)) < 0.1] = -10
    v = np.arange(H)[:, None]
    ground = np.clip(np.round(0.35 * (v - 0.45 * H) * D / (0.55 * H)), 2, D - 8)
    return d, (v > 0.45 * H) & (field == ground)


@pytest.mark.parametrize("seed", range(1000, 1006))
def test_recovers_a_known_ground(sv, seed):
    """The field's ground is d = 0.2172 (v - 168.75): vh = 168.75, qb = 4 * 0.2172 * 206 = 178.3 in the search's terms.  Both step
    settings return (168, 178) on all six seeds, with S between 136 501 and 174 009; between 97.7 % and 98.3 % of the true ground's valid
    pixels are labelled ground with g_tol = 4 (the bar is 90 %)."""
    d, truth = _noisy_truth(seed)
    for step in (1, 2):
        got = sv.ground(d, D, vh_step=step, qb_step=step, tol=2, g_tol=4)
        share = float((got["labels"][truth & (d > 0)] == 1).mean())
        print("seed %d steps (%d, %d): ground %s, ground share %.4f" % (seed, step, step, got["ground"].tolist(), share))
        assert tuple(got["ground"][:2]) == TRUTH, (seed, step, got["ground"])
        assert 136501 <= got["ground"][2] <= 174009 and got["ground"][3] == (d > 0).sum()
        assert share >= 0.9, (seed, step, share)
        assert (got["free_row"] >= 0).all()  # the far background (d = 2 above the horizon) stands on the ground in every column


def _rig_Q(eng):
    """The rig's Q for the default (KITTI) calibration at 1242 x 375, on the host."""
    L = eng.lib()
    L.sv_debug_stereo_rectify.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    Q = np.zeros(16)
    yml = os.path.join(os.path.dirname(eng.LIB_PATH), "stereo_vision", "data", "kitti_2011_09_26.yml").encode()
    assert L.sv_debug_stereo_rectify(yml, W, H, 1.0, 1, Q.ctypes.data, None) == 0
    return Q.reshape(4, 4)


def test_ground_pose_and_points(sv, eng):
    Q = _rig_Q(eng)
    f, cy, base = float(Q[2, 3]), -float(Q[1, 3]), 1.0 / abs(float(Q[3, 2]))
    assert f > 100 and 0 < cy < H and 0.4 < base < 0.7  # a focal length in pixels, a principal row inside the image, KITTI's 0.54 m
    for vh, qb in (TRUTH, (150, 400), (-40, 90), (373, 1)):
        den = 374 - vh
        slope = qb / (4.0 * den)
        pitch = math.atan((cy - vh) / f)
        height = base * math.cos(pitch) / slope
        got = sv.ground_pose(Q, vh, qb, H)
        assert all(isinstance(x, float) for x in got)
        assert np.allclose(got, (height, pitch, slope), rtol=1e-14, atol=0)
    # a level camera 1.65 m above a plane: d(v) = (b / h) (v - cy), so slope = b / h and the horizon is row cy
    Ql = np.array([[1, 0, 0, -600.0], [0, 1, 0, -170.0], [0, 0, 0, 700.0], [0, 0, 1 / 0.5, 0]])
    height, pitch, slope = sv.ground_pose(Ql, 170, round(4 * (0.5 / 1.65) * 204), H)
    assert pitch == 0 and abs(height - 1.65) < 0.01 and abs(slope - 0.5 / 1.65) < 1e-3
    for bad in ((-1, -1), (374, 5), (100, 0)):
        with pytest.raises(ValueError):
            sv.ground_pose(Q, bad[0], bad[1], H)
    # the points: reproject()'s arithmetic on (u, free_row, free_disp), NaN for a column without an obstacle
    rows, disps = np.array([[-1, 200, 374, 0]], np.int32), np.array([[0, 8.5, 40, 0.25]], np.float32)
    XR, XT = sv.CAMERA_TO_VEHICLE, np.array([0.5, 0.0, 1.65])
    P = sv.free_space_points(Ql, rows, disps)
    assert P.shape == (1, 4, 3) and np.isnan(P[0, 0]).all()
    for u in (1, 2, 3):
        w = float(disps[0, u]) / 0.5
        assert P[0, u].tolist() == [(u - 600.0) / w, (rows[0, u] - 170.0) / w, 700.0 / w]
    Pv = sv.free_space_points(Ql, rows[0], disps[0], XR, XT)
    assert Pv.shape == (4, 3) and np.allclose(Pv[1:], P[0, 1:] @ XR.T + XT, rtol=1e-15) and np.isnan(Pv[0]).all()


def _spec(eng, height=8, reserved=None, **kw):
    p = dict(n_bins=64, vh_lo=0, vh_hi=height - 2, vh_step=2, qb_step=2, tol=2, g_tol=4, min_run=8, min_support=0)
    p.update(kw)
    sp = eng.SvGroundSpec()
    for k, v in p.items():
        setattr(sp, k, v)
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


def _bad_specs(eng):
    words = [dict(n_bins=7), dict(n_bins=4097), dict(n_bins=-64), dict(vh_lo=-32769), dict(vh_lo=5, vh_hi=4), dict(vh_hi=7), dict(vh_hi=2 ** 31 - 1), dict(vh_step=0),
             dict(vh_step=-2), dict(qb_step=0), dict(qb_step=64), dict(qb_step=-1), dict(tol=-1), dict(tol=17), dict(g_tol=-1), dict(g_tol=4097), dict(min_run=0),
             dict(min_run=-8), dict(min_support=-1)]
    return [_spec(eng, reserved=k) for k in range(7)] + [_spec(eng, **kw) for kw in words]


def test_validation_needs_no_device(eng):
    """Every SV_ERR_ARG case on host buffers: the checks run before any HIP call, so nothing is read or written; batch == 0 returns
    SV_OK with nothing enqueued.  The workspace is 8 bytes per candidate horizon row and 4 (n_bins + 1) per map row, per pair."""
    L = eng.ground_lib()
    ws = lambda sp, b, w, h: L.sv_ground_workspace_bytes(ctypes.byref(sp) if sp is not None else None, b, w, h)  # noqa: E731
    assert ws(_spec(eng), 2, 16, 8) == 2 * (8 * 4 + 4 * 8 * 65) and ws(_spec(eng), 0, 16, 8) == 0
    assert ws(_spec(eng, vh_lo=-32768, vh_step=1, n_bins=4096), 1, 3, 8) == 8 * (32768 + 7) + 4 * 8 * 4097
    assert ws(_spec(eng, height=32768), 1, 65535, 32768) == 8 * 16384 + 4 * 32768 * 65
    for sp in _bad_specs(eng) + [None]:
        assert ws(sp, 2, 16, 8) == SIZE_MAX
    for b, w, h in ((-1, 16, 8), (65536, 16, 8), (2, 0, 8), (2, 16, 0), (2, 65536, 32768), (2, 16, 32769), (2, -4, -4), (2, 16, 7)):  # height 7: vh_hi = 6 > 5
        assert ws(_spec(eng), b, w, h) == SIZE_MAX
    bufs = {k: np.full(16384, 0x5A, np.uint8) for k in ("disp", "vdisp", "ground", "labels", "free_row", "free_disp", "ws")}
    ptr = lambda name: bufs[name].ctypes.data  # noqa: E731
    good = dict(disp=ptr("disp"), batch=2, width=16, height=8, spec=_spec(eng), vdisp=ptr("vdisp"), ground=ptr("ground"), labels=ptr("labels"),
                free_row=ptr("free_row"), free_disp=ptr("free_disp"), ws=ptr("ws"), ws_bytes=ws(_spec(eng), 2, 16, 8))
    assert ptr("ws") % 8 == 0

    def call(**kw):
        a = dict(good, **kw)
        sp = ctypes.byref(a["spec"]) if a["spec"] is not None else None
        return L.sv_ground_disparity_device(a["disp"], a["batch"], a["width"], a["height"], sp, a["vdisp"], a["ground"], a["labels"], a["free_row"], a["free_disp"],
                                            a["ws"], a["ws_bytes"], None)

    cases = [dict(spec=None), dict(disp=None), dict(ground=None), dict(batch=-1), dict(batch=65536), dict(width=0), dict(height=0), dict(width=-5),
             dict(width=65536, height=32768), dict(height=32769), dict(height=7), dict(ws=None), dict(ws_bytes=good["ws_bytes"] - 1), dict(ws_bytes=0),
             dict(ws=ptr("ws") + 4), dict(disp=ptr("disp") + 2), dict(vdisp=ptr("vdisp") + 1), dict(ground=ptr("ground") + 2), dict(free_row=ptr("free_row") + 3),
             dict(free_disp=ptr("free_disp") + 1)]
    cases += [dict(spec=sp) for sp in _bad_specs(eng)]
    assert len(cases) == 20 + 7 + 19
    for kw in cases:
        rc, text = call(**kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_ground"), (sorted(kw), rc, text)
    assert call(batch=0) == 0 and call(batch=0, ws=None, ws_bytes=0) == 0
    assert all((b == 0x5A).all() for b in bufs.values())
    for bad in (dict(n_bins=7), dict(disp_max=1024), dict(vh_lo=-32769), dict(vh_hi=374), dict(vh_step=0), dict(qb_step=0), dict(qb_step=516), dict(tol=17),
                dict(g_tol=-1), dict(min_run=0), dict(min_support=-1), dict(tol=0.5), dict(vh_step=2 ** 31)):
        with pytest.raises(ValueError):
            eng.ground_spec(H, **dict(dict(disp_max=D), **bad))
    with pytest.raises(ValueError):
        eng.ground_spec(H)  # neither disp_max nor n_bins
    sp = eng.ground_spec(H, D, vh_lo=-5, tol=3, min_support=W)
    assert [getattr(sp, k) for k, _ in sp._fields_[:9]] == [516, -5, 373, 2, 2, 3, 4, 8, W] and list(sp.reserved) == [0] * 7 and ctypes.sizeof(sp) == 64


def test_header_build_and_loader_agree(eng):
    """The header declares the spec's words in the order of the ctypes structure, the library exports the two entries the header
    declares, and build.py lists the new sources and header."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct sv_ground_spec \{(.*?)\} sv_ground_spec;", src, flags=re.S).group(1)
    words = [w.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for w in decl.split(",")]
    assert words == [k for k, _ in eng.SvGroundSpec._fields_[:-1]] + ["reserved[7]"]
    declared = set(re.findall(r"\b(sv_ground_[a-z_]+)\s*\(", src))
    assert declared == {"sv_ground_workspace_bytes", "sv_ground_disparity_device"}
    L = eng.ground_lib()
    assert all(hasattr(L, n) for n in declared)
    assert len(L.sv_ground_disparity_device.argtypes) == 13 and L.sv_ground_workspace_bytes.restype is ctypes.c_size_t
    build = util.pkg("build")
    assert "ground_kernels.hip" in build.SOURCES and "ground.cpp" in build.SOURCES and "ground_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("ground_kernels.hip", "ground.cpp", "ground_kernels.h"))


# ---------------------------------------------------------------------------------------------------------------- GPU

def _gpu(eng, d, disp_max=None, **kw):
    """engine.ground_from_disparity on a numpy batch -> dict of numpy arrays (vdisp as uint32)."""
    res = eng.ground_from_disparity(_cuda(np.asarray(d, np.float32)), disp_max, **kw)
    out = {k: getattr(res, k) for k in OUTPUTS}
    assert all(t is None or t.is_cuda for t in out.values())
    out = {k: None if t is None else t.cpu().numpy() for k, t in out.items()}
    if out["vdisp"] is not None:
        out["vdisp"] = out["vdisp"].view(np.uint32)
    return out


def _check(sv, eng, d, disp_max=None, **kw):
    """GPU == definition for every map of the batch d, all five outputs, exactly; returns the ground records."""
    d = np.asarray(d, np.float32)
    d = d[None] if d.ndim == 2 else d
    got = _gpu(eng, d, disp_max, **kw)
    assert got["vdisp"].dtype == np.uint32 and got["ground"].dtype == np.int32 and got["labels"].dtype == np.uint8
    assert got["free_row"].dtype == np.int32 and got["free_disp"].dtype == np.float32
    for b in range(d.shape[0]):
        want = sv.ground(d[b], disp_max, **kw)
        assert got["ground"][b].tolist() == want["ground"].tolist(), (b, kw, got["ground"][b], want["ground"])
        for k in OUTPUTS:
            assert _bits(got[k][b], want[k]), (b, k, kw)
    return got["ground"]


def _random_map(rng, h, w, density, top=60.0):
    d = rng.uniform(0.05, top, (h, w)).astype(np.float32)
    d[rng.random((h, w)) < 0.2] = np.float32(rng.integers(1, int(4 * top))) / 4 + np.float32(0.125)  # ties of the rounding
    bad = rng.random((h, w)) >= density
    d[bad] = rng.choice(np.array([NAN, -10.0, 0.0, -0.0, -INF], np.float32), int(bad.sum()))
    return d


def _scene(rng, h, w, top=60.0, density=0.9):
    """A ground ramp with obstacles as runs of constant disparity in a few columns, noise and holes: long runs of one bin per row."""
    v = np.arange(h, dtype=np.float32)[:, None]
    d = np.maximum(top * (v - 0.4 * h) / (0.6 * h), 1.0) * np.ones((1, w), np.float32)
    for _ in range(max(1, w // 40)):
        x0, ww = int(rng.integers(0, w)), int(rng.integers(1, max(2, w // 6)))
        y0, hh = int(rng.integers(0, h)), int(rng.integers(1, max(2, h // 2)))
        d[y0:y0 + hh, x0:x0 + ww] = np.float32(rng.uniform(2, top))
    d = (d + rng.normal(0, 0.2, (h, w))).astype(np.float32)
    d[rng.random((h, w)) >= density] = -10
    return d


@pytest.fixture(scope="module")
def engine_maps(eng):
    """The engine's own D1 (disp_max 127: D = 128): the committed KITTI pair 0 and the synthetic pairs 1000 .. 1002."""
    synth = util.pkg("synth")
    entry = util.digests()["kitti0_d128"]
    L0, R0 = util.case_images(entry)
    batch = synth.make_batch(1000, 3)
    lefts, rights = np.stack([L0] + list(batch[:, 0])), np.stack([R0] + list(batch[:, 1]))
    e = eng.StereoEngine(W, H, eng.SvParams.driver(127), chunk=4, n_slots=2, n_workers=3)
    try:
        d1, _, _ = e.process_host(np.ascontiguousarray(lefts), np.ascontiguousarray(rights))
    finally:
        e.close()
    assert util.sha(d1[0]) == entry["stages"]["final1"]
    return np.ascontiguousarray(d1)


@pytest.mark.gpu
def test_engine_maps_equal_the_definition(sv, eng, engine_maps):
    rec = _check(sv, eng, engine_maps, 127)
    print("ground records of KITTI pair 0 and synthetic pairs 1000 .. 1002:", rec.tolist())
    assert (rec[:, 1] > 0).all() and (rec[:, 2] >= W).all() and rec[0, 3] == (engine_maps[0] > 0).sum()
    _check(sv, eng, engine_maps[:2], 127, vh_step=1, qb_step=1, tol=0, g_tol=0, min_run=1)
    _check(sv, eng, engine_maps[:2], 127, vh_lo=-200, vh_hi=300, vh_step=5, qb_step=5, tol=16, g_tol=12, min_run=3)


@pytest.mark.gpu
def test_semantic_ground_of_a_synthetic_pair(sv, eng, engine_maps):
    """The ground fitted to the engine's D1 of synthetic pairs against the fit of their truth field, (168, 178).  The admissible
    distance is what the CPU oracle's D1 (oracle/pyoracle.py, bit-identical to the engine's) gave for seeds 1000 .. 1005 with the
    default spec (steps 2, tol 2), plus one search step of 2.  Observed, the same for disp_max 127 and 255:
        seeds 1000, 1003, 1004, 1005: (168, 178); seeds 1001, 1002: (168, 176) - distance 0 in vh, at most 2 in qb.
    So |vh - 168| <= 0 + 2 and |qb - 178| <= 2 + 2.  The share of the truth's ground pixels that are labelled ground is printed."""
    rec = _gpu(eng, engine_maps[1:], 127)
    for i, seed in enumerate((1000, 1001, 1002)):
        vh, qb = rec["ground"][i][:2]
        print("seed %d: engine ground (%d, %d), truth fit %s" % (seed, vh, qb, TRUTH))
        assert abs(vh - TRUTH[0]) <= 2 and abs(qb - TRUTH[1]) <= 4, (seed, vh, qb)
        _, truth = _noisy_truth(seed)
        found = truth & (engine_maps[1 + i] > 0)
        share = float((rec["labels"][i][found] == 1).mean())
        print("seed %d: %.4f of the true ground's valid pixels are labelled ground" % (seed, share))  # reported, no bar is set for it


@pytest.mark.gpu
def test_random_maps_and_densities(sv, eng):
    rng = np.random.default_rng(41)
    for density in (0.0, 0.01, 0.5, 1.0):
        maps = np.stack([_random_map(rng, 47, 331, density), _scene(rng, 47, 331, density=density)])
        rec = _check(sv, eng, maps, 63, min_support=0)
        if density == 0.0:
            assert rec[:, 2:].tolist() == [[0, 0], [0, 0]]
        _check(sv, eng, maps, 63, vh_step=1, qb_step=1, min_run=2)  # min_support = the width
    # +inf is valid and lands in the last bin; a map of one value
    _check(sv, eng, np.full((9, 70), INF, np.float32), 15, min_run=2)
    _check(sv, eng, np.full((9, 70), 7.25, np.float32), 15, min_run=2, vh_lo=-30)


@pytest.mark.gpu
def test_shapes_around_the_tiling(sv, eng):
    rng = np.random.default_rng(43)
    for w in (1, 63, 64, 65, 1242):
        for h in (2, 3, 375):
            d = _scene(rng, h, w, top=30.0)
            kw = dict(min_run=min(2, h), min_support=0)
            if h == 375 and w == 1242:
                kw.update(vh_step=4, qb_step=4)
            _check(sv, eng, d, 31, **kw)
    for h, w in ((8, 255), (9, 256), (17, 257), (16, 513), (7, 1)):  # around the histogram's 256 pixels per sweep and 8 rows per strip
        _check(sv, eng, np.stack([_scene(rng, h, w, top=30.0) for _ in range(3)]), 31, min_run=2, vh_step=1, qb_step=1)


@pytest.mark.gpu
def test_spec_words(sv, eng):
    rng = np.random.default_rng(47)
    d = np.stack([_scene(rng, 120, 300, top=40.0), _random_map(rng, 120, 300, 0.7, top=40.0)])
    far = np.stack([_scene(rng, 120, 300, top=1000.0), _random_map(rng, 120, 300, 0.7, top=1100.0)])  # reaches and passes bin 4095
    _check(sv, eng, d, n_bins=44)  # saturates: most of the scene lands in bin 43
    _check(sv, eng, far, n_bins=4096, vh_step=7, qb_step=9)
    _check(sv, eng, far, n_bins=4096, vh_lo=100, vh_hi=100, qb_step=1)
    _check(sv, eng, d, 40, vh_lo=-300, vh_hi=60)
    _check(sv, eng, d, 40, vh_lo=-32768, vh_hi=-32700, vh_step=1)
    for step in (1, 2, 5):
        _check(sv, eng, d, 40, vh_step=step, qb_step=step)
    _check(sv, eng, d, 40, vh_step=1000, qb_step=163)  # one candidate of each
    for tol in (0, 16):
        _check(sv, eng, d, 40, tol=tol)
    for g_tol in (0, 4096):
        _check(sv, eng, d, 40, g_tol=g_tol)
    for min_run in (1, 3, 120, 121, 2 ** 31 - 1):
        rec = _gpu(eng, d, 40, min_run=min_run)
        _check(sv, eng, d, 40, min_run=min_run)
        if min_run > 120:
            assert (rec["free_row"] == -1).all() and (rec["free_disp"] == 0).all()
    none = _check(sv, eng, d, 40, min_support=2 ** 31 - 1)
    assert none[:, :2].tolist() == [[-1, -1], [-1, -1]]


@pytest.mark.gpu
def test_a_4k_frame(sv, eng):
    rng = np.random.default_rng(53)
    d = _scene(rng, 2160, 3840, top=180.0)
    rec = _check(sv, eng, d, 255, vh_lo=700, vh_hi=1000, vh_step=10, qb_step=8)
    assert rec[0, 1] > 0 and abs(rec[0, 0] - 864) <= 10, rec


@pytest.mark.gpu
def test_no_ground_in_a_mixed_batch(sv, eng):
    rng = np.random.default_rng(59)
    maps = np.stack([_scene(rng, 90, 200, top=30.0), np.full((90, 200), -10, np.float32), _scene(rng, 90, 200, top=30.0),
                     rng.choice(np.array([NAN, 0.0, -INF], np.float32), (90, 200))])
    rec = _check(sv, eng, maps, 31, min_run=2)
    assert rec[1].tolist() == [-1, -1, 0, 0] and rec[3].tolist() == [-1, -1, 0, 0] and rec[0, 1] > 0 and rec[2, 1] > 0
    got = _gpu(eng, maps, 31, min_run=2)
    assert not got["labels"][[1, 3]].any() and not got["vdisp"][[1, 3]].any() and (got["free_row"][[1, 3]] == -1).all() and (got["labels"][[0, 2]] == 1).any()


def _raw(eng, d_t, spec, vdisp, ground, labels, free_row, free_disp, ws=None, stream=None):
    """The C entry on caller-owned buffers (torch tensors)."""
    import torch
    L = eng.ground_lib()
    B, Hh, Ww = d_t.shape
    n = L.sv_ground_workspace_bytes(ctypes.byref(spec), B, Ww, Hh)
    assert n != SIZE_MAX
    if ws is None:
        ws = torch.empty((n // 8 + 1,), dtype=torch.int64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = L.sv_ground_disparity_device(d_t.data_ptr(), B, Ww, Hh, ctypes.byref(spec), ptr(vdisp), ground.data_ptr(), ptr(labels), ptr(free_row), ptr(free_disp),
                                      ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream if stream is None else stream)
    assert rc == 0, (rc, L.sv_last_error(None))
    return ws


@pytest.mark.gpu
def test_batches_repeats_and_workspace(sv, eng, engine_maps):
    import torch
    rng = np.random.default_rng(61)
    maps = np.concatenate([engine_maps, _scene(rng, H, W)[None], np.where(engine_maps[:1] > 20, engine_maps[:1], np.float32(-10))])
    batch = _gpu(eng, maps, 127)
    assert len({tuple(r) for r in batch["ground"].tolist()}) == len(maps)
    for b in range(len(maps)):
        alone = _gpu(eng, maps[b:b + 1], 127)
        assert all(_bits(alone[k][0], batch[k][b]) for k in OUTPUTS), b
    again = _gpu(eng, maps, 127)
    assert all(_bits(again[k], batch[k]) for k in OUTPUTS)
    # the workspace's contents do not matter: all zeros, all ones, and the leftovers of another call
    t = _cuda(maps)
    spec = eng.ground_spec(H, 127, min_support=W)
    n = eng.ground_lib().sv_ground_workspace_bytes(ctypes.byref(spec), len(maps), W, H)
    for fill in (0, -1, 0x5A5A5A5A5A5A5A5A):
        ws = torch.full((n // 8 + 1,), fill, dtype=torch.int64, device="cuda")
        out = [torch.empty(s, dtype=dt, device="cuda") for s, dt in (((len(maps), H, spec.n_bins), torch.int32), ((len(maps), 4), torch.int32), ((len(maps), H, W), torch.uint8),
                                                                    ((len(maps), W), torch.int32), ((len(maps), W), torch.float32))]
        _raw(eng, t, spec, *out, ws=ws)
        _raw(eng, t[:2].contiguous(), eng.ground_spec(H, 127, vh_step=1, qb_step=1), None, torch.empty((2, 4), dtype=torch.int32, device="cuda"), None, None, None, ws=ws)
        _raw(eng, t, spec, *out, ws=ws)
        torch.cuda.synchronize()
        assert all(_bits(o.cpu().numpy(), batch[k]) for o, k in zip(out, OUTPUTS)), fill
    # an empty batch: nothing is enqueued, empty outputs
    res = eng.ground_from_disparity(torch.empty((0, 8, 16), device="cuda"), 15)
    assert tuple(res.ground.shape) == (0, 4) and tuple(res.vdisp.shape) == (0, 8, 64) and tuple(res.labels.shape) == (0, 8, 16) and tuple(res.free_row.shape) == (0, 16)
    # 300 small maps, one frame without a batch axis, and the engine layer's input checks
    rec = _check(sv, eng, np.stack([_scene(rng, 23, 41, top=15.0) for _ in range(300)]), 15, min_run=2, vh_step=1, qb_step=1)
    assert len({tuple(r) for r in rec.tolist()}) > 20
    one = eng.ground_from_disparity(t[0], 127)
    assert tuple(one.ground.shape) == (1, 4) and _bits(one.labels.cpu().numpy()[0], batch["labels"][0])
    for bad in (dict(disp=t.double()), dict(disp=t.cpu()), dict(disp=t[0, 0]), dict(disp_max=None), dict(disp_max=2000), dict(vh_hi=H - 1), dict(tol=17), dict(min_run=0)):
        with pytest.raises(ValueError):
            eng.ground_from_disparity(**dict(dict(disp=t, disp_max=127), **bad))


@pytest.mark.gpu
def test_nullable_outputs(eng, engine_maps):
    """Each output left out leaves the others unchanged, and nothing is written through a pointer that was not given: poisoned
    buffers stay poisoned."""
    import torch
    full = _gpu(eng, engine_maps, 127)
    flags = {"vdisp": ("want_vdisp",), "labels": ("want_labels",), "free": ("want_free",)}
    for name, (flag,) in flags.items():
        part = _gpu(eng, engine_maps, 127, **{flag: False})
        gone = ("free_row", "free_disp") if name == "free" else (name,)
        for k in OUTPUTS:
            assert (part[k] is None) if k in gone else _bits(part[k], full[k]), (name, k)
    only = _gpu(eng, engine_maps, 127, want_vdisp=False, want_labels=False, want_free=False)
    assert _bits(only["ground"], full["ground"]) and all(only[k] is None for k in OUTPUTS if k != "ground")
    # the C entry with free_row but no free_disp, and the reverse
    t = _cuda(engine_maps)
    B = len(engine_maps)
    spec = eng.ground_spec(H, 127, min_support=W)
    for keep in ("free_row", "free_disp"):
        ground = torch.empty((B, 4), dtype=torch.int32, device="cuda")
        row = torch.full((B, W), -77, dtype=torch.int32, device="cuda")
        dsp = torch.full((B, W), -7.25, dtype=torch.float32, device="cuda")
        _raw(eng, t, spec, None, ground, None, row if keep == "free_row" else None, dsp if keep == "free_disp" else None)
        torch.cuda.synchronize()
        assert _bits(ground.cpu().numpy(), full["ground"])
        if keep == "free_row":
            assert _bits(row.cpu().numpy(), full["free_row"]) and (dsp == -7.25).all().item()
        else:
            assert _bits(dsp.cpu().numpy(), full["free_disp"]) and (row == -77).all().item()


@pytest.mark.gpu
def test_on_torch_current_stream(eng, engine_maps):
    """The input written by torch ops on a busy side stream and a dependent torch op behind the call, no explicit synchronisation in
    between: the results are those of the input at rest."""
    import torch
    want = _gpu(eng, engine_maps, 127)
    src = _cuda(engine_maps)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        x = torch.randn(4096, 4096, device="cuda")
        for _ in range(4):
            x = x @ x  # keeps the stream busy while the host runs ahead
        d = torch.zeros_like(src)
        d.copy_(src)
        res = eng.ground_from_disparity(d, 127)
        total = res.labels.sum(dtype=torch.int64) + res.ground.sum()  # dependent ops on the same stream
    torch.cuda.synchronize()
    del x
    got = {k: getattr(res, k).cpu().numpy() for k in OUTPUTS}
    assert all(_bits(got[k], want[k]) for k in OUTPUTS)
    assert total.item() == int(want["labels"].sum(dtype=np.int64)) + int(want["ground"].sum())


@pytest.mark.gpu
def test_rig_ground(sv, eng):
    import torch
    rigmod = util.pkg("rig")
    ls = np.stack([util.load_png("kitti0_color_left.png"), np.repeat(util.load_png("kitti1_left.png")[..., None], 3, -1)])
    rs = np.stack([util.load_png("kitti0_color_right.png"), np.repeat(util.load_png("kitti1_right.png")[..., None], 3, -1)])
    bgr_l, bgr_r = np.ascontiguousarray(ls[..., ::-1]), np.ascontiguousarray(rs[..., ::-1])
    rig = rigmod.StereoRig(W, H)
    try:
        tl, tr = _cuda(bgr_l), _cuda(bgr_r)
        res = rig.ground(tl, tr, transform=(sv.CAMERA_TO_VEHICLE, None))
        gl, gr = rig.frontend(tl, tr)
        d1, _ = rig.engine.process_device(gl, gr, want_d2=False)
        assert torch.equal(d1, rig.disparity(tl, tr))
        ref = eng.ground_from_disparity(d1, rig.params.disp_max)
        assert ref.spec.n_bins == 1024 and ref.spec.min_support == W
        for k in OUTPUTS:
            assert isinstance(getattr(res, k), torch.Tensor) and torch.equal(getattr(res, k), getattr(ref, k)), k
        rec = res.ground.cpu().numpy()
        print("rig ground records:", rec.tolist(), "poses:", res.pose)
        assert (rec[:, 1] > 0).all()
        for b in range(2):
            assert res.pose[b] == sv.ground_pose(rig.Q, int(rec[b, 0]), int(rec[b, 1]), H)
        assert 1.3 < res.pose[0][0] < 2.0 and abs(res.pose[0][1]) < 0.2  # KITTI's cameras are 1.65 m above the road, nearly level (the golden map gives 1.63 m)
        want_pts = sv.free_space_points(rig.Q, res.free_row.cpu().numpy(), res.free_disp.cpu().numpy(), sv.CAMERA_TO_VEHICLE, None)
        assert isinstance(res.points, np.ndarray) and res.points.shape == (2, W, 3) and _bits(res.points, want_pts)
        hit = res.free_row.cpu().numpy() >= 0
        assert hit.sum() > W and (res.points[hit][:, 0] > 0).all() and np.isnan(res.points[~hit]).all()  # forward of the camera
        # the definition on the same maps
        want = sv.ground(d1[0].cpu().numpy(), rig.params.disp_max)
        assert all(_bits(getattr(res, k)[0].cpu().numpy().view(want[k].dtype), want[k]) for k in OUTPUTS)
        # numpy in: numpy out; spec words and output flags pass through
        out = rig.ground(bgr_l, bgr_r, vh_step=4, qb_step=4, min_run=4, want_vdisp=False, transform="rig")
        ref = eng.ground_from_disparity(d1, rig.params.disp_max, vh_step=4, qb_step=4, min_run=4)
        assert out.vdisp is None and all(isinstance(getattr(out, k), np.ndarray) for k in OUTPUTS[1:])
        assert all(_bits(getattr(out, k), getattr(ref, k).cpu().numpy()) for k in OUTPUTS[1:])
        assert _bits(out.points, sv.free_space_points(rig.Q, out.free_row, out.free_disp, rig.XR, rig.XT))
        for bad in (dict(tol=17), dict(vh_hi=H), dict(min_run=0), dict(transform="sideways"), dict(n_bins=64), dict(want_free=False), dict(qb_step=0)):
            with pytest.raises(ValueError):
                rig.ground(bgr_l, bgr_r, **bad)
    finally:
        rig.close()
    p = util.pkg("engine").SvParams.driver(255)
    p.subsampling = 1
    half = rigmod.StereoRig(W, H, params=p)
    try:
        with pytest.raises(ValueError):
            half.ground(bgr_l, bgr_r)
    finally:
        half.close()
