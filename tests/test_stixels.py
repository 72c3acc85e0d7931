"""Stixels and detector-free object boxes (include/stereo_vision_hip.h (H)): the numpy definition in stereo_vision.sv on a hand-built
map, its identity with the free space of (G), synthetic scenes with known rectangles, the C ABI's argument checks, and the HIP kernels
- C entry, engine and rig layers - against the definition.

Everything is compared exactly.  That is derived, not chosen: the only floating-point operations between a disparity and any of the
five outputs are 4.0f * d (exact: a power of two) and the rounding of that product to an integer (round half to even on both sides);
the rest is integer comparison and addition."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_ground import _bits, _noisy_truth

SV_ERR_ARG = -1
SIZE_MAX = 2 ** 64 - 1
NAN, INF = float("nan"), float("inf")
W, H, D = 1242, 375, 128
OUTPUTS = ("stixels", "n_stixels", "boxes", "info", "counts")
WORDS = ("q_min", "sim", "max_gap", "min_rows", "max_layers", "col_step", "sim_cols", "min_cols")


# ---------------------------------------------------------------------------------------------------------------- CPU

# 14 rows x 9 columns, written bottom-up per column (the first entry is row 13), 16 bins, q_min 4, sim 2, max_gap 1, min_rows 3,
# max_layers 2.  A number is a bin q under a label 2 (d = q / 4); X is a pixel that matches in disparity (d = 2: q = 8) but is
# labelled ground; the other letters carry a label 2 over something that is not a disparity or saturates.
X, N_, M_, S_, T_ = "X", "nan", "-10", "100", "inf"
HAND_COLS = [
    [8, X, 8, 8, X, X, 8, 8, 8, X, X, X, X, X],          # a gap of max_gap rows bridged, one of max_gap + 1 ends the run
    [8, 12, 8, 12, 8, 12, 12, X, X, X, X, X, X, X],      # bridged rows (12) are not visited again: they would make (12, 7, 12, 4)
    [8, 13, 8, 13, 13, 13, X, X, X, X, X, X, X, X],      # a run one row short of min_rows consumes its bridged row 12, not the rows above t
    [4, 4, 4, 3, 3, 3, X, X, X, X, X, X, X, X],          # q = q_min kept, q_min - 1 dropped (it would match: |3 - 4| <= sim)
    [8, 10, 10, 11, 11, 11, 11, X, X, X, X, X, X, X],    # |q - qb| = sim kept, sim + 1 ends the run
    [6, 7, 8, 9, 10, 11, 12, 13, X, X, X, X, X, X],      # a ramp: neighbour to neighbour it would be one run, base to base it is three
    [S_, 50, N_, 15, M_, X, T_, T_, N_, T_, X, X, X, X],  # label 2 over NaN and -10 is not foreground; 100, 12.5, 3.75 and inf share bin 15
    [8, 8, 8, X, X, 8, 8, 8, X, X, 8, 8, 8, X],          # three stixels, max_layers 2
    [X, X, X, X, X, X, X, X, X, X, X, X, X, X],          # none
]
HAND_SPEC = dict(n_bins=16, q_min=4, sim=2, max_gap=1, min_rows=3, max_layers=2)
HAND_STIXELS = [[(13, 10, 8, 3), (7, 5, 8, 3)], [(13, 9, 8, 3)], [(10, 8, 13, 3)], [(13, 11, 4, 3)], [(13, 11, 8, 3), (10, 7, 11, 4)],
                [(13, 11, 6, 3), (10, 8, 9, 3)], [(13, 10, 15, 3), (7, 4, 15, 3)], [(13, 11, 8, 3), (8, 6, 8, 3)], []]
HAND_COUNTS = [2, 1, 1, 1, 2, 2, 2, 3, 0]

# the first layer of 14 visited columns, written out: three objects, a split at sim_cols + 1 = 3, a segment one column short of
# min_cols = 3, an even count for the lower median
NONE = (-1, -1, -1, -1)
HAND_LAYER0 = np.array([(20, 10, 10, 11), (21, 12, 11, 10), (19, 8, 13, 12), (20, 5, 16, 16), (22, 6, 16, 17), (20, 7, 18, 14), NONE, (20, 10, 20, 11),
                        (20, 10, 20, 11), NONE, (15, 3, 30, 13), (16, 4, 32, 13), (17, 5, 34, 13), (18, 6, 36, 13)], np.int32)
HAND_BOXES = {1: [(0, 8, 3, 14), (3, 5, 3, 18), (10, 3, 4, 16)], 2: [(0, 8, 5, 14), (6, 5, 5, 18), (20, 3, 7, 16)], 3: [(0, 8, 7, 14), (9, 5, 7, 18), (30, 3, 10, 16)]}
HAND_INFO = [(3, 10, 13, 11), (3, 16, 18, 16), (4, 30, 36, 32)]


def _hand_map():
    d, lab = np.zeros((14, 9), np.float32), np.zeros((14, 9), np.uint8)
    special = {N_: NAN, M_: -10.0, S_: 100.0, T_: INF}
    for u, col in enumerate(HAND_COLS):
        for k, e in enumerate(col):
            v = 13 - k
            if e == X:
                d[v, u], lab[v, u] = 2.0, (1, 3, 0)[(u + k) % 3]
            elif e in special:
                d[v, u], lab[v, u] = special[e], 2
            else:
                d[v, u], lab[v, u] = e / 4.0, 2
    return d, lab


def _want_hand(columns, max_layers=2):
    st, n = np.full((max_layers, len(columns), 4), -1, np.int32), np.zeros(len(columns), np.int32)
    for i, u in enumerate(columns):
        n[i] = HAND_COUNTS[u]
        for k, s in enumerate(HAND_STIXELS[u][:max_layers]):
            st[k, i] = s
    return st, n


def test_hand_built_map(sv):
    d, lab = _hand_map()
    for step in (1, 2, 3, 9, 100):
        st, n = sv.stixels(d, lab, col_step=step, **HAND_SPEC)
        want_st, want_n = _want_hand(range(0, 9, step))
        assert st.dtype == np.int32 and n.dtype == np.int32 and st.shape == want_st.shape
        assert np.array_equal(n, want_n) and np.array_equal(st, want_st), (step, n.tolist(), st.tolist())
    # in column 6 the run (7, 4, 15, 3) bridges a NaN; with max_layers 1 it is counted but not stored
    st, n = sv.stixels(d, lab, **dict(HAND_SPEC, max_layers=1))
    assert np.array_equal(n, HAND_COUNTS) and np.array_equal(st, _want_hand(range(9), 1)[0])
    # the objects of the written-out first layer
    for step, boxes in HAND_BOXES.items():
        for cap, rows in ((None, 3), (0, 0), (1, 1), (3, 3), (5, 3)):
            bx, info, count = sv.stixel_objects(HAND_LAYER0, col_step=step, sim_cols=2, min_cols=3, capacity=cap)
            assert count == 3 and bx.dtype == np.int32 and info.dtype == np.int32 and bx.shape == (rows, 4) and info.shape == (rows, 4)
            assert bx.tolist() == [list(b) for b in boxes[:rows]] and info.tolist() == [list(r) for r in HAND_INFO[:rows]], (step, cap)
    assert sv.stixel_objects(HAND_LAYER0, sim_cols=2, min_cols=2)[2] == 4        # the two-column segment is kept
    assert sv.stixel_objects(HAND_LAYER0, sim_cols=3, min_cols=3)[0].tolist()[0] == [0, 5, 6, 18]  # no split at |16 - 13| = sim_cols
    assert sv.stixel_objects(HAND_LAYER0, sim_cols=2, min_cols=5)[2] == 0
    # the objects of the hand-built map: every column but the last has a stixel; bases 8 8 13 4 8 6 15 8 -
    bx, info, count = sv.stixel_objects(sv.stixels(d, lab, **HAND_SPEC)[0][0], sim_cols=2, min_cols=2)
    assert count == 2 and bx.tolist() == [[0, 9, 2, 5], [4, 11, 2, 3]] and info.tolist() == [[2, 8, 8, 8], [2, 6, 8, 6]]
    for bad in (dict(n_bins=7), dict(n_bins=4097), dict(q_min=-1), dict(q_min=4096), dict(sim=-1), dict(sim=4097), dict(max_gap=-1), dict(max_gap=256),
                dict(min_rows=0), dict(max_layers=0), dict(max_layers=65), dict(col_step=0), dict(sim_cols=-1), dict(sim_cols=4097), dict(min_cols=0),
                dict(sim=1.5), dict(min_rows=True), dict(col_step=2 ** 31)):
        with pytest.raises(ValueError):
            sv.stixels(d, lab, **dict(HAND_SPEC, **bad))
    with pytest.raises(ValueError):
        sv.stixels(d, lab[:5], **HAND_SPEC)
    with pytest.raises(ValueError):
        sv.stixel_objects(HAND_LAYER0, capacity=-1)


def _identity(sv, d, disp_max, min_run):
    g = sv.ground(d, disp_max, min_run=min_run)
    nb = g["vdisp"].shape[1]
    st, n = sv.stixels(d, g["labels"], n_bins=nb, sim=nb, q_min=0, max_gap=0, col_step=1, min_rows=min_run, max_layers=1)
    assert np.array_equal(st[0, :, 0], g["free_row"]), (disp_max, min_run)
    assert np.array_equal(n > 0, g["free_row"] >= 0)
    return g["free_row"]


@pytest.mark.parametrize("seed", range(1000, 1006))
def test_first_stixel_is_the_free_space(sv, seed):
    """With sim >= n_bins, q_min 0, max_gap 0, col_step 1 and min_rows = min_run the first layer's v_bottom is free_row, -1 included."""
    d, _ = _noisy_truth(seed)
    row = _identity(sv, d, D, 8)
    assert (row >= 0).all()
    d[:, 100:140] = -10  # columns without an obstacle
    assert (_identity(sv, d, D, 3)[100:140] == -1).all()


def test_first_stixel_is_the_free_space_of_the_golden_map(sv):
    d = np.load(os.path.join(util.ROOT, "tests", "golden", "kitti0_d128.npz"))["final1"].astype(np.float32).reshape(H, W)
    _identity(sv, d, 127, 8)


SCENE_SPECS = ((6, 8), (8, 10))  # (sim, sim_cols)
SCENE_SPEC = dict(q_min=16, min_rows=8, min_cols=16, max_gap=2)


def _truth_scene(seed):
    """(map, [(x0, w, foot, h, dd)] x 5): the ground of synth.disparity_field, five rectangles in disjoint column ranges standing on it
    (disparity = the ground's at the foot row plus 0 .. 2, rows foot - h .. foot - 1), N(0, 0.3) noise, 10 % of the pixels invalid."""
    rng = np.random.default_rng(seed)
    v = np.arange(H)
    ground = np.clip(np.round(0.35 * (v - 0.45 * H) * D / (0.55 * H)), 2, D - 8)
    field = np.repeat(ground[:, None], W, 1)
    rects = []
    for k in range(5):
        x0 = 60 + 230 * k + int(rng.integers(0, 40))
        w, foot, h = int(rng.integers(60, 160)), int(rng.integers(230, 340)), int(rng.integers(50, 150))
        dd = float(ground[foot]) + int(rng.integers(0, 3))
        field[foot - h:foot, x0:x0 + w] = dd
        rects.append((x0, w, foot, h, dd))
    d = (field + rng.normal(0, 0.3, (H, W))).astype(np.float32)
    d[rng.random((H, W)) < 0.1] = -10
    return d, rects


@pytest.mark.parametrize("seed", range(12))
def test_recovers_known_rectangles(sv, seed):
    """Five rectangles on a known ground come back as exactly five objects: left edge, right edge and top within 2 pixels of the truth,
    the bottom within 8 rows of the foot on either side (above: the rectangle's rows within g_tol / 4 = 1 px of a ground that rises
    0.217 px per row are labelled ground; below: a noisy ground pixel under the foot can be labelled obstacle, lie within sim of the
    rectangle and become the base), q_med / 4 within 0.5 px of the rectangle's disparity.
    Observed with the committed numpy form, seeds 0 .. 11, (sim, sim_cols) = (6, 8) and (8, 10): five objects every time; left edge,
    right edge and top off by 0 pixels; the box's bottom between 5 rows above and 3 rows below the rectangle's; q_med / 4 off by at
    most 0.25 px."""
    d, rects = _truth_scene(seed)
    g = sv.ground(d, D)
    for sim, sim_cols in SCENE_SPECS:
        st, _ = sv.stixels(d, g["labels"], D, sim=sim, **{k: v for k, v in SCENE_SPEC.items() if k != "min_cols"})
        boxes, info, count = sv.stixel_objects(st[0], sim_cols=sim_cols, min_cols=SCENE_SPEC["min_cols"])
        margins = [(int(b[0]) - r[0], int(b[0] + b[2]) - (r[0] + r[1]), int(b[1]) - (r[2] - r[3]), int(b[1] + b[3]) - r[2], float(i[3]) / 4 - r[4])
                   for b, i, r in zip(boxes, info, rects)]
        print("seed %d sim %d sim_cols %d: %d objects, (left, right, top, bottom, q_med / 4) - truth: %s" % (seed, sim, sim_cols, count, margins))
        assert count == 5 and len(boxes) == 5, (seed, sim, count, boxes.tolist())
        for left, right, top, bottom, dq in margins:
            assert abs(left) <= 2 and abs(right) <= 2 and abs(top) <= 2 and abs(bottom) <= 8 and abs(dq) <= 0.5, (seed, sim, margins)
    world = sv.stixel_world(d, D, sim=sim, sim_cols=sim_cols, **SCENE_SPEC)
    assert np.array_equal(world["stixels"][:st.shape[0]], st) and np.array_equal(world["boxes"], boxes) and world["count"] == 5
    assert np.array_equal(world["labels"], g["labels"]) and np.array_equal(world["ground"], g["ground"])


def _spec(eng, reserved=None, **kw):
    p = dict(n_bins=64, q_min=16, sim=6, max_gap=2, min_rows=8, max_layers=8, col_step=1, sim_cols=8, min_cols=16)
    p.update(kw)
    sp = eng.SvStixelSpec()
    for k, v in p.items():
        setattr(sp, k, v)
    if reserved is not None:
        sp.reserved[reserved] = 1
    return sp


def _bad_specs(eng):
    words = [dict(n_bins=7), dict(n_bins=4097), dict(n_bins=-64), dict(q_min=-1), dict(q_min=4096), dict(sim=-1), dict(sim=4097), dict(max_gap=-1), dict(max_gap=256),
             dict(min_rows=0), dict(min_rows=-8), dict(max_layers=0), dict(max_layers=65), dict(col_step=0), dict(col_step=-2), dict(sim_cols=-1), dict(sim_cols=4097),
             dict(min_cols=0), dict(min_cols=-1)]
    return [_spec(eng, reserved=k) for k in range(7)] + [_spec(eng, **kw) for kw in words]


def test_validation_needs_no_device(eng):
    """Every SV_ERR_ARG case on host buffers: the checks run before any HIP call, so nothing is read or written; batch == 0 returns
    SV_OK with nothing enqueued.  The workspace is 16 bytes per visited column, per pair."""
    L = eng.stixel_lib()
    ws = lambda sp, b, w, h: L.sv_stixel_workspace_bytes(ctypes.byref(sp) if sp is not None else None, b, w, h)  # noqa: E731
    assert ws(_spec(eng), 2, 16, 8) == 2 * 16 * 16 and ws(_spec(eng), 0, 16, 8) == 0
    assert ws(_spec(eng, col_step=3), 5, 16, 8) == 5 * 6 * 16 and ws(_spec(eng, col_step=2 ** 31 - 1), 1, 65535, 32768) == 16
    assert ws(_spec(eng), 1, 2 ** 31 - 1, 1) == 16 * (2 ** 31 - 1)
    for sp in _bad_specs(eng) + [None]:
        assert ws(sp, 2, 16, 8) == SIZE_MAX
    for b, w, h in ((-1, 16, 8), (65536, 16, 8), (2, 0, 8), (2, 16, 0), (2, 65536, 32768), (2, 16, 32769), (2, -4, -4)):
        assert ws(_spec(eng), b, w, h) == SIZE_MAX
    raw = {k: np.full(16384 + 16, 0x5A, np.uint8) for k in ("disp", "labels", "stixels", "n_stixels", "boxes", "info", "counts", "ws")}
    bufs = {k: a[(-a.ctypes.data) % 16:][:16384] for k, a in raw.items()}
    ptr = lambda name: bufs[name].ctypes.data  # noqa: E731
    assert all(ptr(k) % 16 == 0 for k in bufs)
    good = dict(disp=ptr("disp"), labels=ptr("labels"), batch=2, width=16, height=8, spec=_spec(eng), capacity=4, stixels=ptr("stixels"), n_stixels=ptr("n_stixels"),
                boxes=ptr("boxes"), info=ptr("info"), counts=ptr("counts"), ws=ptr("ws"), ws_bytes=ws(_spec(eng), 2, 16, 8))

    def call(**kw):
        a = dict(good, **kw)
        sp = ctypes.byref(a["spec"]) if a["spec"] is not None else None
        return L.sv_stixel_disparity_device(a["disp"], a["labels"], a["batch"], a["width"], a["height"], sp, a["capacity"], a["stixels"], a["n_stixels"], a["boxes"],
                                            a["info"], a["counts"], a["ws"], a["ws_bytes"], None)

    cases = [dict(spec=None), dict(disp=None), dict(labels=None), dict(counts=None), dict(batch=-1), dict(batch=65536), dict(width=0), dict(height=0), dict(width=-5),
             dict(width=65536, height=32768), dict(height=32769), dict(capacity=-1), dict(ws=None), dict(ws_bytes=good["ws_bytes"] - 1), dict(ws_bytes=0),
             dict(ws=ptr("ws") + 8), dict(disp=ptr("disp") + 2), dict(n_stixels=ptr("n_stixels") + 1), dict(counts=ptr("counts") + 2), dict(stixels=ptr("stixels") + 4),
             dict(boxes=ptr("boxes") + 8), dict(info=ptr("info") + 12)]
    cases += [dict(spec=sp) for sp in _bad_specs(eng)]
    assert len(cases) == 22 + 7 + 19
    for kw in cases:
        rc, text = call(**kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_stixel"), (sorted(kw), rc, text)
    assert call(batch=0) == 0 and call(batch=0, ws=None, ws_bytes=0) == 0
    assert all((b == 0x5A).all() for b in raw.values())
    for bad in (dict(n_bins=7), dict(disp_max=1024), dict(q_min=4096), dict(sim=4097), dict(max_gap=256), dict(min_rows=0), dict(max_layers=65), dict(col_step=0),
                dict(sim_cols=-1), dict(min_cols=0), dict(sim=0.5), dict(col_step=2 ** 31)):
        with pytest.raises(ValueError):
            eng.stixel_spec(**dict(dict(disp_max=D), **bad))
    with pytest.raises(ValueError):
        eng.stixel_spec()  # neither disp_max nor n_bins
    sp = eng.stixel_spec(D, sim=3, col_step=2)
    assert [getattr(sp, k) for k, _ in sp._fields_[:9]] == [516, 16, 3, 2, 8, 8, 2, 8, 16] and list(sp.reserved) == [0] * 7 and ctypes.sizeof(sp) == 64


def test_header_build_and_loader_agree(eng):
    """The header declares the spec's words in the order of the ctypes structure, the library exports the two entries the header
    declares, and build.py lists the new sources and header."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct sv_stixel_spec \{(.*?)\} sv_stixel_spec;", src, flags=re.S).group(1)
    words = [w.strip() for decl in re.findall(r"int32_t ([^;]+);", body) for w in decl.split(",")]
    assert words == [k for k, _ in eng.SvStixelSpec._fields_[:-1]] + ["reserved[7]"]
    declared = set(re.findall(r"\b(sv_stixel_[a-z_]+)\s*\(", src))
    assert declared == {"sv_stixel_workspace_bytes", "sv_stixel_disparity_device"}
    L = eng.stixel_lib()
    assert all(hasattr(L, n) for n in declared)
    assert len(L.sv_stixel_disparity_device.argtypes) == 15 and L.sv_stixel_workspace_bytes.restype is ctypes.c_size_t
    build = util.pkg("build")
    assert "stixel_kernels.hip" in build.SOURCES and "stixels.cpp" in build.SOURCES and "stixel_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("stixel_kernels.hip", "stixels.cpp", "stixel_kernels.h"))


# ---------------------------------------------------------------------------------------------------------------- GPU

def _gpu(eng, d, lab, disp_max=None, capacity=64, **kw):
    """engine.stixels_from_disparity on numpy batches -> dict of numpy arrays."""
    res = eng.stixels_from_disparity(_cuda(np.asarray(d, np.float32)), _cuda(np.asarray(lab, np.uint8)), disp_max, capacity=capacity, **kw)
    out = {k: getattr(res, k) for k in OUTPUTS}
    assert all(t is None or t.is_cuda for t in out.values())
    return {k: None if t is None else t.cpu().numpy() for k, t in out.items()}


def _want(sv, d, lab, disp_max=None, capacity=64, **kw):
    """The definition for one map, in the engine layer's shapes: boxes and info padded with 0 to the capacity."""
    st, n = sv.stixels(d, lab, disp_max, **kw)
    p = sv.stixel_params(disp_max, **kw)
    bx, info, count = sv.stixel_objects(st[0], p["col_step"], p["sim_cols"], p["min_cols"], capacity)
    pad = lambda a: np.concatenate([a, np.zeros((capacity - len(a), 4), np.int32)])  # noqa: E731
    return {"stixels": st, "n_stixels": n, "boxes": pad(bx), "info": pad(info), "counts": np.int32(count)}


def _check(sv, eng, d, lab, disp_max=None, capacity=64, **kw):
    """GPU == definition for every map of the batch, all five outputs, exactly; returns the counts."""
    d, lab = np.asarray(d, np.float32), np.asarray(lab, np.uint8)
    if d.ndim == 2:
        d, lab = d[None], lab[None]
    got = _gpu(eng, d, lab, disp_max, capacity, **kw)
    assert all(got[k].dtype == np.int32 for k in OUTPUTS)
    for b in range(d.shape[0]):
        want = _want(sv, d[b], lab[b], disp_max, capacity, **kw)
        for k in OUTPUTS:
            assert _bits(got[k][b], want[k]), (b, k, kw, got[k][b].tolist() if got[k][b].size < 200 else got[k][b].shape)
    return got["counts"]


def _labels(eng, d, disp_max, **kw):
    """The labels of (G) for a numpy batch, from the GPU (tests/test_ground.py holds them to the definition)."""
    return eng.ground_from_disparity(_cuda(np.asarray(d, np.float32)), disp_max, want_vdisp=False, want_free=False, **kw).labels.cpu().numpy()


def _random_world(rng, h, w, top=30.0):
    """A map of vertical strips of a few disparities with noise and holes, and labels that are mostly 2."""
    d = np.zeros((h, w), np.float32)
    for u in range(w):
        v = 0
        while v < h:
            n = int(rng.integers(1, max(2, h // 3)))
            d[v:v + n, u] = np.float32(rng.integers(4, int(4 * top))) / 4
            v += n
    d[:, rng.random(w) < 0.5] = np.float32(rng.integers(8, 60)) / 4  # half of the columns share one disparity: objects
    d = d + (rng.integers(-2, 3, (h, w)) / np.float32(4)).astype(np.float32)
    bad = rng.random((h, w)) < 0.15
    d[bad] = rng.choice(np.array([NAN, -10.0, 0.0, 0.125, INF], np.float32), int(bad.sum()))
    lab = np.where(rng.random((h, w)) < 0.85, 2, rng.integers(0, 4, (h, w))).astype(np.uint8)
    return d, lab


@pytest.mark.gpu
def test_hand_built_map_on_the_gpu(sv, eng):
    d, lab = _hand_map()
    for step in (1, 2, 3):
        got = _gpu(eng, d[None], lab[None], col_step=step, sim_cols=2, min_cols=2, **HAND_SPEC)
        want_st, want_n = _want_hand(range(0, 9, step))
        assert np.array_equal(got["stixels"][0], want_st) and np.array_equal(got["n_stixels"][0], want_n), step
        _check(sv, eng, d, lab, col_step=step, sim_cols=2, min_cols=2, **HAND_SPEC)
    assert got["counts"].tolist() == [0]
    got = _gpu(eng, d[None], lab[None], sim_cols=2, min_cols=2, capacity=3, **HAND_SPEC)
    assert got["counts"].tolist() == [2] and got["boxes"][0].tolist() == [[0, 9, 2, 5], [4, 11, 2, 3], [0, 0, 0, 0]] and got["info"][0, :2].tolist() == [[2, 8, 8, 8], [2, 6, 8, 6]]
    # the written-out first layer as a map of one row per stixel is not possible; its objects are reached through maps below


@pytest.mark.gpu
def test_truth_scenes_on_the_gpu(sv, eng):
    maps, rects = zip(*[_truth_scene(seed) for seed in (0, 1, 2)])
    maps = np.stack(maps)
    lab = _labels(eng, maps, D)
    for sim, sim_cols in SCENE_SPECS:
        counts = _check(sv, eng, maps, lab, D, sim=sim, sim_cols=sim_cols, **SCENE_SPEC)
        assert counts.tolist() == [5, 5, 5]


@pytest.fixture(scope="module")
def real_maps(eng):
    """The engine's D1 of the seven committed real pairs (tests/golden/profile_*) at disp_max 127 and 255: [(name, disp_max, d1)]."""
    out = []
    for name in ("aloe", "cones", "raindeer", "urban1", "urban2", "urban3", "urban4"):
        l, r = util.load_png("profile_%s_left.png" % name), util.load_png("profile_%s_right.png" % name)
        for disp_max in (127, 255):
            e = eng.StereoEngine(l.shape[1], l.shape[0], eng.SvParams.driver(disp_max), chunk=1, n_slots=2, n_workers=2)
            try:
                d1, _, _ = e.process_host(np.ascontiguousarray(l[None]), np.ascontiguousarray(r[None]))
            finally:
                e.close()
            out.append((name, disp_max, np.ascontiguousarray(d1[0])))
    return out


@pytest.mark.gpu
def test_real_frames_equal_the_definition(sv, eng, real_maps):
    for name, disp_max, d1 in real_maps:
        lab = _labels(eng, d1[None], disp_max)
        counts = _check(sv, eng, d1, lab[0], disp_max)
        got = _gpu(eng, d1[None], lab, disp_max)
        print("%s disp_max %d: %d objects, %d stixels, at most %d in a column" % (name, disp_max, counts[0], got["n_stixels"].sum(), got["n_stixels"].max()))
    name, disp_max, d1 = real_maps[6]
    lab = _labels(eng, d1[None], disp_max)[0]
    _check(sv, eng, d1, lab, disp_max, sim=4, q_min=0, max_gap=0, min_rows=1, max_layers=3, col_step=2, sim_cols=2, min_cols=2, capacity=7)


@pytest.mark.gpu
def test_uniform_maps(sv, eng):
    """All obstacle, no obstacle, and "no ground" (every valid pixel is labelled 3)."""
    d = np.full((40, 130), 6.0, np.float32)
    for fill, n_obj in ((2, 1), (1, 0), (3, 0), (0, 0)):
        counts = _check(sv, eng, d, np.full(d.shape, fill, np.uint8), 31)
        assert counts.tolist() == [n_obj]
    got = _gpu(eng, d[None], np.full((1,) + d.shape, 2, np.uint8), 31)
    assert got["boxes"][0, 0].tolist() == [0, 0, 130, 40] and got["info"][0, 0].tolist() == [130, 24, 24, 24] and (got["stixels"][0, 0] == [39, 0, 24, 40]).all()
    assert (got["stixels"][0, 1:] == -1).all() and (got["n_stixels"] == 1).all()
    rng = np.random.default_rng(3)
    noise = rng.uniform(0.05, 30, (40, 130)).astype(np.float32)
    lab = _labels(eng, noise[None], 31, min_support=2 ** 31 - 1)  # no ground
    assert (lab == 3).all()
    assert _check(sv, eng, noise, lab[0], 31).tolist() == [0]


@pytest.mark.gpu
def test_shapes_around_the_tiling(sv, eng):
    rng = np.random.default_rng(71)
    small = dict(q_min=8, sim=3, max_gap=1, min_rows=3, max_layers=4, sim_cols=3, min_cols=2)
    for w in (1, 63, 64, 65, 255, 257, 3840):
        for h in (1, 2, 3, 4, 24):  # min_rows 3: heights min_rows - 1 and min_rows + 1 among them
            if w == 3840 and h not in (2, 24):
                continue
            d, lab = _random_world(rng, h, w)
            for step in (1, 2, 7):
                _check(sv, eng, d, lab, 31, col_step=step, **small)
    d, lab = _random_world(rng, 4, 70)
    for min_rows in (1, 3, 4, 5):
        _check(sv, eng, d, lab, 31, **dict(small, min_rows=min_rows))


@pytest.mark.gpu
def test_spec_words(sv, eng):
    rng = np.random.default_rng(73)
    d, lab = zip(*[_random_world(rng, 90, 300, top=40.0) for _ in range(2)])
    d, lab = np.stack(d), np.stack(lab)
    base = dict(q_min=8, sim=3, max_gap=1, min_rows=3, max_layers=4, sim_cols=3, min_cols=2)
    for kw in (dict(q_min=0), dict(q_min=4095), dict(sim=0), dict(sim=4096), dict(max_gap=0), dict(max_gap=255), dict(min_rows=1), dict(min_rows=2 ** 31 - 1),
               dict(max_layers=1), dict(max_layers=64), dict(col_step=299), dict(col_step=2 ** 31 - 1), dict(sim_cols=0), dict(sim_cols=4096), dict(min_cols=1),
               dict(min_cols=2 ** 31 - 1)):
        _check(sv, eng, d, lab, 40, **dict(base, **kw))
    _check(sv, eng, d, lab, n_bins=44, **base)  # saturates: most of the map lands in bin 43
    _check(sv, eng, d * 30, lab, n_bins=4096, **base)
    for capacity in (0, 1, 2, 1000):
        _check(sv, eng, d, lab, 40, capacity=capacity, **base)


@pytest.mark.gpu
def test_alternating_rows(sv, eng):
    """A column of one-row runs - the most stixels a column can have: every second row foreground (max_gap 0, min_rows 1), and every
    row foreground with alternating disparities (sim 0)."""
    h, w = 101, 66
    d = np.full((h, w), 5.0, np.float32)
    lab = np.full((h, w), 2, np.uint8)
    lab[::2] = 1
    got = _gpu(eng, d[None], lab[None], 31, q_min=0, sim=0, max_gap=0, min_rows=1, max_layers=64)
    assert (got["n_stixels"] == 50).all() and (got["stixels"][0, 49, :, 0] == 1).all() and (got["stixels"][0, 50:] == -1).all()
    _check(sv, eng, d, lab, 31, q_min=0, sim=0, max_gap=0, min_rows=1, max_layers=64)
    d[::2] = 9.0
    lab[:] = 2
    got = _gpu(eng, d[None], lab[None], 31, q_min=0, sim=0, max_gap=0, min_rows=1, max_layers=8)
    assert (got["n_stixels"] == 101).all()
    _check(sv, eng, d, lab, 31, q_min=0, sim=0, max_gap=0, min_rows=1, max_layers=8)
    _check(sv, eng, d, lab, 31, q_min=0, sim=0, max_gap=1, min_rows=2, max_layers=8)  # each run bridges the other disparity's rows


@pytest.mark.gpu
def test_batches_do_not_matter(sv, eng):
    rng = np.random.default_rng(79)
    worlds = [_random_world(rng, 60, 200) for _ in range(64)]
    d, lab = np.stack([x[0] for x in worlds]), np.stack([x[1] for x in worlds])
    kw = dict(q_min=8, sim=3, max_gap=1, min_rows=3, max_layers=4, sim_cols=3, min_cols=2, capacity=16)
    full = _gpu(eng, d, lab, 31, **kw)
    assert len(set(full["counts"].tolist())) > 3 and full["counts"].max() > 16  # more objects than rows somewhere
    for b in (0, 5, 63):
        alone = _gpu(eng, d[b:b + 1], lab[b:b + 1], 31, **kw)
        assert all(_bits(alone[k][0], full[k][b]) for k in OUTPUTS), b
    three = _gpu(eng, d[[7, 0, 33]], lab[[7, 0, 33]], 31, **kw)
    assert all(_bits(three[k], full[k][[7, 0, 33]]) for k in OUTPUTS)
    again = _gpu(eng, d, lab, 31, **kw)
    assert all(_bits(again[k], full[k]) for k in OUTPUTS)
    _check(sv, eng, d[:6], lab[:6], 31, **kw)
    import torch
    res = eng.stixels_from_disparity(torch.empty((0, 8, 16), device="cuda"), torch.empty((0, 8, 16), dtype=torch.uint8, device="cuda"), 15)
    assert tuple(res.stixels.shape) == (0, 8, 16, 4) and tuple(res.boxes.shape) == (0, 64, 4) and tuple(res.counts.shape) == (0,)
    one = eng.stixels_from_disparity(_cuda(d[0]), _cuda(lab[0]), 31, **kw)
    assert tuple(one.counts.shape) == (1,) and _bits(one.stixels.cpu().numpy()[0], full["stixels"][0])
    t, l = _cuda(d), _cuda(lab)
    for bad in (dict(d1=t.double()), dict(d1=t.cpu()), dict(labels=l.int()), dict(labels=l[:, :5]), dict(disp_max=None), dict(sim=4097), dict(capacity=-1), dict(col_step=0)):
        with pytest.raises(ValueError):
            eng.stixels_from_disparity(**dict(dict(d1=t, labels=l, disp_max=31), **bad))


def _raw(eng, d_t, lab_t, spec, capacity, stixels, n_stixels, boxes, info, counts, ws=None):
    """The C entry on caller-owned buffers (torch tensors)."""
    import torch
    L = eng.stixel_lib()
    B, Hh, Ww = d_t.shape
    n = L.sv_stixel_workspace_bytes(ctypes.byref(spec), B, Ww, Hh)
    assert n != SIZE_MAX
    if ws is None:
        ws = torch.empty((n // 8 + 1,), dtype=torch.int64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = L.sv_stixel_disparity_device(d_t.data_ptr(), lab_t.data_ptr(), B, Ww, Hh, ctypes.byref(spec), capacity, ptr(stixels), ptr(n_stixels), ptr(boxes), ptr(info),
                                      counts.data_ptr(), ws.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, L.sv_last_error(None))
    return ws


@pytest.mark.gpu
def test_c_entry_nullable_outputs_and_untouched_rows(sv, eng):
    """Each output left out leaves the others unchanged; rows of boxes and info at and beyond counts, and everything beyond the
    capacity, keep the caller's bytes; the layers beyond a column's count are -1; the workspace's contents do not matter."""
    import torch
    rng = np.random.default_rng(83)
    worlds = [_random_world(rng, 50, 150) for _ in range(3)]
    d, lab = np.stack([x[0] for x in worlds]), np.stack([x[1] for x in worlds])
    kw = dict(q_min=8, sim=3, max_gap=1, min_rows=3, max_layers=5, sim_cols=3, min_cols=2)
    spec = eng.stixel_spec(31, **kw)
    t, l = _cuda(d), _cuda(lab)
    B, cap, POISON = 3, 20, -77
    want = [_want(sv, d[b], lab[b], 31, capacity=1000, **kw) for b in range(B)]
    assert min(int(w["counts"]) for w in want) < cap < max(int(w["counts"]) for w in want)  # both sides of the capacity

    def buffers():
        return {"stixels": torch.full((B, 5, 150, 4), POISON, dtype=torch.int32, device="cuda"), "n_stixels": torch.full((B, 150), POISON, dtype=torch.int32, device="cuda"),
                "boxes": torch.full((B, cap + 1, 4), POISON, dtype=torch.int32, device="cuda"), "info": torch.full((B, cap + 1, 4), POISON, dtype=torch.int32, device="cuda"),
                "counts": torch.full((B,), POISON, dtype=torch.int32, device="cuda")}

    def verify(out, gone=()):
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in out.items()}
        for k in gone:
            assert (got[k] == POISON).all(), k
        for b in range(B):
            n = min(int(want[b]["counts"]), cap)
            assert got["counts"][b] == want[b]["counts"]
            if "stixels" not in gone:
                assert _bits(got["stixels"][b], want[b]["stixels"])
            if "n_stixels" not in gone:
                assert _bits(got["n_stixels"][b], want[b]["n_stixels"])
            for k in ("boxes", "info"):
                if k not in gone:
                    # [B, cap + 1, 4] viewed as the call's [B, cap, 4]: pair b's rows start at 4 * cap * b words
                    flat = got[k].reshape(-1)[4 * cap * b:4 * cap * (b + 1)].reshape(cap, 4)
                    assert _bits(flat[:n], want[b][k][:n]), (b, k)
                    assert (flat[n:] == POISON).all(), (b, k)
        for k in ("boxes", "info"):
            if k not in gone:
                assert (got[k].reshape(-1)[4 * cap * B:] == POISON).all()

    out = buffers()
    _raw(eng, t, l, spec, cap, *[out[k] for k in OUTPUTS])
    verify(out)
    for k in OUTPUTS[:-1]:
        out = buffers()
        _raw(eng, t, l, spec, cap, *[None if name == k else out[name] for name in OUTPUTS])
        verify(out, gone=(k,))
    out = buffers()
    _raw(eng, t, l, spec, cap, None, None, None, None, out["counts"])
    verify(out, gone=OUTPUTS[:-1])
    n = eng.stixel_lib().sv_stixel_workspace_bytes(ctypes.byref(spec), B, 150, 50)
    for fill in (0, -1, 0x5A5A5A5A5A5A5A5A):
        out = buffers()
        _raw(eng, t, l, spec, cap, *[out[k] for k in OUTPUTS], ws=torch.full((n // 8 + 1,), fill, dtype=torch.int64, device="cuda"))
        verify(out)
    out = buffers()  # capacity 0: counts alone
    _raw(eng, t, l, spec, 0, out["stixels"], out["n_stixels"], out["boxes"], out["info"], out["counts"])
    torch.cuda.synchronize()
    assert (out["boxes"] == POISON).all().item() and (out["info"] == POISON).all().item() and out["counts"].cpu().tolist() == [int(w["counts"]) for w in want]
    # the engine layer's flags
    full = _gpu(eng, d, lab, 31, capacity=cap, **kw)
    part = _gpu(eng, d, lab, 31, capacity=cap, want_stixels=False, **kw)
    assert part["stixels"] is None and part["n_stixels"] is None and all(_bits(part[k], full[k]) for k in OUTPUTS[2:])
    part = _gpu(eng, d, lab, 31, capacity=cap, want_objects=False, **kw)
    assert part["boxes"] is None and part["info"] is None and all(_bits(part[k], full[k]) for k in ("stixels", "n_stixels", "counts"))


@pytest.mark.gpu
def test_rig_objects_and_the_chain_into_box_positions(sv, eng):
    """rig.objects == ground_from_disparity + stixels_from_disparity + box_positions_from_disparity on the rig's d1 == the numpy
    definition; the device-side chain (boxes and counts never leave the device) equals the host-side one (boxes read back, passed in
    again, n_boxes from counts)."""
    import torch
    rigmod = util.pkg("rig")
    ls = np.stack([util.load_png("kitti0_color_left.png"), np.repeat(util.load_png("kitti1_left.png")[..., None], 3, -1)])
    rs = np.stack([util.load_png("kitti0_color_right.png"), np.repeat(util.load_png("kitti1_right.png")[..., None], 3, -1)])
    bgr_l, bgr_r = np.ascontiguousarray(ls[..., ::-1]), np.ascontiguousarray(rs[..., ::-1])
    rig = rigmod.StereoRig(W, H)
    try:
        tl, tr = _cuda(bgr_l), _cuda(bgr_r)
        C2V = (sv.CAMERA_TO_VEHICLE, None)
        for cap in (64, 3):
            res = rig.objects(tl, tr, transform=C2V, capacity=cap)
            d1 = rig.disparity(tl, tr)
            g = eng.ground_from_disparity(d1, rig.params.disp_max)
            ref = eng.stixels_from_disparity(d1, g.labels, rig.params.disp_max, capacity=cap)
            assert ref.spec.n_bins == 1024
            for k in OUTPUTS:
                assert isinstance(getattr(res, k), torch.Tensor) and torch.equal(getattr(res, k), getattr(ref, k)), k
            assert torch.equal(res.ground.labels, g.labels) and torch.equal(res.ground.ground, g.ground)
            counts = res.counts.cpu().numpy()
            print("rig.objects capacity %d: counts %s, boxes of pair 0 %s" % (cap, counts.tolist(), res.boxes[0, :min(cap, counts[0])].cpu().tolist()))
            assert (counts >= 0).all() and counts.max() > 0
            # the definition on the same maps
            for b in range(2):
                want = _want(sv, d1[b].cpu().numpy(), g.labels[b].cpu().numpy(), rig.params.disp_max, capacity=cap)
                assert all(_bits(getattr(res, k)[b].cpu().numpy(), want[k]) for k in OUTPUTS), b
            # host-side chain: boxes and counts read back and passed in again
            boxes_h, n_h = res.boxes.cpu().numpy().copy(), np.minimum(counts, cap)
            pos_h, stat_h = eng.box_positions_from_disparity(d1, rig.Q, boxes_h, n_h, XR=sv.CAMERA_TO_VEHICLE, select="near", disparity="d1")
            assert tuple(res.positions.shape) == (2, cap, 3) and res.positions.dtype == torch.float64
            assert _bits(res.positions.cpu().numpy(), pos_h.cpu().numpy()) and _bits(res.stat.cpu().numpy(), stat_h.cpu().numpy())
            pos_np, stat_np = sv.box_positions(d1.cpu().numpy(), boxes_h, n_h, Q=rig.Q, XR=sv.CAMERA_TO_VEHICLE, select="near", disparity="d1")
            assert _bits(res.positions.cpu().numpy(), pos_np) and _bits(res.stat.cpu().numpy(), stat_np)
            pos = res.positions.cpu().numpy()
            for b in range(2):
                n = int(n_h[b])
                assert np.isnan(pos[b, n:]).all() and np.isfinite(pos[b, :n]).all() and (pos[b, :n, 0] > 0).all()  # forward of the camera
        # numpy in: numpy out; spec words of both layers pass through; positions can be left out
        out = rig.objects(bgr_l, bgr_r, positions=False, vh_step=4, qb_step=4, sim=8, sim_cols=10, col_step=2, max_layers=2)
        g = eng.ground_from_disparity(d1, rig.params.disp_max, vh_step=4, qb_step=4)
        ref = eng.stixels_from_disparity(d1, g.labels, rig.params.disp_max, sim=8, sim_cols=10, col_step=2, max_layers=2)
        assert out.positions is None and all(isinstance(getattr(out, k), np.ndarray) for k in OUTPUTS) and out.stixels.shape == (2, 2, 621, 4)
        assert all(_bits(getattr(out, k), getattr(ref, k).cpu().numpy()) for k in OUTPUTS)
        empty = rig.objects(tl, tr, capacity=0)
        assert tuple(empty.boxes.shape) == (2, 0, 4) and tuple(empty.positions.shape) == (2, 0, 3) and torch.equal(empty.counts, res.counts)
        for bad in (dict(sim=4097), dict(vh_hi=H), dict(min_rows=0), dict(transform="sideways"), dict(n_bins=64), dict(capacity=-1), dict(capacity=65536), dict(col_step=0)):
            with pytest.raises(ValueError):
                rig.objects(bgr_l, bgr_r, **bad)
    finally:
        rig.close()
    p = util.pkg("engine").SvParams.driver(255)
    p.subsampling = 1
    half = rigmod.StereoRig(W, H, params=p)
    try:
        with pytest.raises(ValueError):
            half.objects(bgr_l, bgr_r)
    finally:
        half.close()
