"""The kernels whose per-lane work was cut to what differs between lanes - k_raster_tiles (16-byte tile clear, two rows per trip of the
atomicMax loop, one column pair per thread in the tile store), k_lr2<false> (the check in integers) and k_gap_rows (lane masks built once,
scalar word loop) - at the map sizes where their new paths turn over, against the oracle's stages on keep_debug handles, byte for byte.
(k_ccl_border's scalar word index changes no path: the speckle cases of test_postprocess_edges.py cover it.)  One more test runs the two
k_support instantiations (four and eight wavefronts per lattice point) on the shape that separates them.

raster   widths 64, 65, 126, 127, 130 (even: 8-byte stores, odd: 4-byte; last tile 64, 1, 62, 63 and 2 columns wide) x heights 31, 32, 33,
         63, 70 (last tile row 31, 32, 1, 31 and 6 rows high; the engine refuses maps of 31 rows, which only the oracle sees), lattices painted
         densely with the image corners added so that every tile above the map's last row is drawn into; 130 x 70 once more with a
         tile-list cap of 1: the tiles walk all triangles.
L/R      painted WTA maps (postprocess_cases._lr: d = 0, u - d = 0 | -1, u + d = W - 1 | W, partners exactly lr_threshold apart and one
         more, -1 and -10 entries) at the even widths 66 and 130 with lr_threshold 0 and 2, one odd width (k_lr) and one half-resolution
         map (k_lr2<true>).
gaps     widths 64, 65, 128, 130 x ipol_gap_width 3, 5000 x add_corners 0, 1: rows without a valid pixel, gaps that start / end at
         bit 0 / 63 of a mask word, gaps over two and three words, leading and trailing gaps, single pixels, noise.
support  20 pairs of 330 x 70 at D = 64 in one chunk (2 x 13 x 20 = 520 workgroups: k_support<false, 4>) and one such pair alone
         (k_support<false, 8>), disp_min 0 and 3: the first lattice columns of a row have ranges clipped per lane, the later ones have not.

CPU: the oracle produces every stage of every case, the painted maps keep the contract of the injection hooks, and each family is what
it says (tile seams drawn into, both verdicts of the L/R check, filled and open gaps)."""
import numpy as np
import pytest

import plane_raster_cases as prc
import postprocess_cases as pc
import util
from pyoracle import ElasParams

RASTER_W, RASTER_H = (64, 65, 126, 127, 130), (31, 32, 33, 63, 70)
CHAIN = ("support", "tri1", "tri2", "planes1", "planes2", "grid1", "grid2", "tri_id1", "tri_id2", "wta1", "wta2")
SEED, SEED_D = 11, 24
_CACHE = {}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.size == b.size and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _once(key, fn):
    """A reference computed once, shared between the tests and left unchanged."""
    if key not in _CACHE:
        out = fn()
        for a in (out.values() if isinstance(out, dict) else out if isinstance(out, (tuple, list)) else [out]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def _pair(H, W):
    return _once(("pair", H, W), lambda: util.pkg("synth").make_pair(SEED, H, W, SEED_D))


# ---- raster -------------------------------------------------------------------------------------------------------------------------------
def _raster_case(W, H):
    """Every lattice point painted, neighbours in a row 2 and in a column 6 apart (the redundancy passes keep them), corners added."""
    Wc, Hc = (W + 4) // 5, (H + 4) // 5
    k, j = np.meshgrid(np.arange(Wc), np.arange(Hc))
    lat = (2 * ((k + 3 * j) % 8)).astype(np.int16)
    lat[0] = 0
    lat[:, 0] = 0
    return prc.Case("trim_%dx%d" % (W, H), "trim", lat, (W, H), dict(add_corners=1), "tile seams of the id map", (), disp_max=63)


def _raster_want(oracle, c):
    return _once(("raster", c.W, c.H), lambda: oracle.chain_from_lattice(prc.params(ElasParams, c), c.lattice, *_pair(c.H, c.W)))


@pytest.mark.parametrize("W", RASTER_W)
def test_raster_cases_draw_into_every_tile(oracle, W):
    for H in RASTER_H:
        c = _raster_case(W, H)
        ch = _raster_want(oracle, c)
        assert len(ch["support"]) >= 3 and set(CHAIN) <= set(ch), (W, H)
        for side in "12":
            ids = ch["tri_id" + side]
            assert ids.shape == (H, W)
            for ty in range(0, H, prc.RT_H):
                for tx in range(0, W, prc.RT_W):
                    t = ids[ty:min(ty + prc.RT_H, H - 1), tx:tx + prc.RT_W]   # (a column piece's row range is half open: the map's last row stays -1)
                    assert t.size == 0 or (t >= 0).any() or (side == "2" and tx > 0), (W, H, side, ty, tx)   # (the right image's triangles end at the last u - d)
            assert (ids[H - 1] == -1).all() and (side == "2" or (ids[:, W - 1] >= 0).any()), (W, H, side)  # the left image is drawn up to its last column
    c = _raster_case(130, 70)
    ch = _raster_want(oracle, c)
    cnt = prc.tile_counts(prc.footprints(ch["support"], ch["tri1"], c.W, c.H, 0), c.W, c.H)
    assert cnt.min() > 1, "with a cap of 1 every tile's list overflows"


@pytest.fixture(scope="module")
def eng():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    util.pkg("build").build()
    return util.pkg("engine")


@pytest.mark.gpu
@pytest.mark.parametrize("W", RASTER_W)
def test_raster_tiles_against_the_oracle(eng, oracle, W):
    for H in RASTER_H:
        c = _raster_case(W, H)
        want = _raster_want(oracle, c)
        L, R = _pair(H, W)
        if H < 32:  # sv_create admits 32 rows and more: a 31-row tile is the last tile row of the 63-row maps
            with pytest.raises(eng.StereoError, match="unsupported image size"):
                eng.StereoEngine(W, H, prc.params(eng.SvParams, c), keep_debug=True, n_workers=2)
            continue
        e = eng.StereoEngine(W, H, prc.params(eng.SvParams, c), keep_debug=True, n_workers=2)
        try:
            e.debug_inject("lattice", np.array(c.lattice))
            for cap in (-1, 1) if (W, H) == (130, 70) else (-1,):
                e.debug_set("rt_cap", cap)
                _, _, status = e.process_host(L, R)
                assert int(status[0]) == len(want["support"]), (W, H, cap, status)
                bad = [k for k in CHAIN if not _same(e.debug(k), want[k].ravel())]
                assert not bad, (W, H, cap, bad)
            e.debug_set("rt_cap", -1)
            e.debug_inject("lattice", None, None)
        finally:
            e.close()


# ---- L/R check ----------------------------------------------------------------------------------------------------------------------------
_LR = {}
for _name, _shape, _sub, _thr in (("even_66_t0", (33, 66), 0, 0), ("even_66_t2", (33, 66), 0, 2), ("even_130_t0", (33, 130), 0, 0), ("even_130_t2", (33, 130), 0, 2),
                                  ("odd_65_t0", (33, 65), 0, 0), ("half_130_t2", (33, 130), 1, 2)):
    _m1, _m2, _e = pc._lr(_shape, _sub, _thr, 100 + len(_LR))
    _LR[_name] = pc.Case("trim_lr_" + _name, "lr", "wta", _m1, _m2, over=dict(lr_threshold=_thr, subsampling=_sub), expect=_e)


def _post_pair(c):
    return _once(("ppair",) + c.image_shape, lambda: util.pkg("synth").make_pair(pc.PAIR_SEED, c.image_shape[0], c.image_shape[1], pc.PAIR_D))


def _post_want(oracle, c):
    return _once(("post", c.name), lambda: pc.chain(oracle, pc.params(ElasParams, c.over), c.stage, c.left, c.right))


def _contract(c):
    for m in (c.left, c.right):
        ok = ((m >= 0) & (m <= pc.DISP_MAX) & (m == np.floor(m))) | (m == -10) | ((m == -1) if c.stage == "wta" else False)
        assert ok.all(), c.name


@pytest.mark.parametrize("name", sorted(_LR))
def test_lr_cases_are_what_they_say(oracle, name):
    c = _LR[name]
    _contract(c)
    assert oracle.run_stages(pc.params(ElasParams, c.over), *_post_pair(c)) >= 3, "the carrier pair must pass the support stage"
    ch = _post_want(oracle, c)
    for side in (0, 1):
        vals = [float(ch["lr%d" % (side + 1)][x[3]]) for x in c.expect if x[0] == "at" and x[2] == side]
        want = [float(x[4]) for x in c.expect if x[0] == "at" and x[2] == side]
        assert vals == want and sum(v >= 0 for v in vals) >= 3 and sum(v < 0 for v in vals) >= 5, (name, side)
        m = c.maps(side)
        assert (m == 0).any() and (m == -1).any() and (m == -10).any(), name


def _run_post(eng, oracle, c):
    """Injects the case, processes the carrier pair and compares every stage behind the injection and the returned maps."""
    want = _post_want(oracle, c)
    L, R = _post_pair(c)
    e = eng.StereoEngine(L.shape[1], L.shape[0], pc.params(eng.SvParams, c.over), keep_debug=True, n_workers=2)
    try:
        e.debug_inject(c.stage, c.left, c.right)
        d1, d2, status = e.process_host(L, R)
        assert int(status[0]) >= 3, (c.name, status)
        got = {s + side: e.debug(s + side).reshape(c.map_shape) for s in pc.STAGES for side in "12"}
        bad = [(k, int((got[k] != want[k]).sum())) for s in pc.STAGES for k in (s + "1", s + "2") if not _same(got[k], want[k])]
        assert not bad, (c.name, bad)
        assert _same(d1[0], want["final1"]) and _same(d2[0], want["final2"]), c.name
        e.debug_inject(c.stage, None, None)
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_LR))
def test_lr_check_against_the_oracle(eng, oracle, name):
    _run_post(eng, oracle, _LR[name])


# ---- gap rows -----------------------------------------------------------------------------------------------------------------------------
GAP_W = (64, 65, 128, 130)
GAP_PARAMS = ((3, 0), (3, 1), (5000, 0), (5000, 1))


def _gap_map(W, H=33):
    M = pc._blank((H, W))

    def seg(v, a, b, val):
        if a < W:
            M[v, a:min(b, W - 1) + 1] = val

    # row 0 stays without a valid pixel
    seg(2, 60, 63, 10), seg(2, 67, 68, 12)       # a gap of 3 from bit 0 of the second word
    seg(4, 59, 60, 10), seg(4, 64, 65, 12)       # ... up to bit 63 of the first
    seg(6, 61, 62, 10), seg(6, 66, 67, 11)       # ... from bit 63
    seg(8, 60, 61, 10), seg(8, 65, 66, 12)       # ... up to bit 0
    seg(10, 58, 60, 10), seg(10, 65, 66, 13)     # a gap of 4 across the words' seam: open at width 3
    seg(12, 10, 10, 9), seg(12, 100, 100, 11)    # over two words
    seg(14, 2, 2, 9), seg(14, W - 1, W - 1, 10)  # over all words of the row: three at 130
    seg(16, 3, 4, 12), seg(16, W - 5, W - 4, 14)  # open at the start and at the end by 3 ...
    seg(18, 4, 5, 12), seg(18, W - 6, W - 5, 14)  # ... and by 4
    seg(20, 0, 0, 8), seg(20, W - 1, W - 1, 9)   # valid at the first and the last pixel only
    seg(22, 63, 63, 7)                           # one valid pixel, at bit 63 ...
    seg(24, 64 if W > 64 else 0, 64 if W > 64 else 0, 7)  # ... and at bit 0
    seg(26, 0, W - 1, 6)                         # nothing to fill
    rng = np.random.default_rng(W)
    M[28:] = np.where(rng.random((H - 28, W)) < 0.5, rng.integers(0, 13, (H - 28, W)).astype(np.float32), pc.INV)
    return M


def _gap_case(W, g, corners):
    return pc.Case("trim_gap_%d_g%d_c%d" % (W, g, corners), "gaps", "lr", _gap_map(W), over=dict(speckle_size=0, ipol_gap_width=g, add_corners=corners))


@pytest.mark.parametrize("W", GAP_W)
def test_gap_cases_are_what_they_say(oracle, W):
    for g, corners in GAP_PARAMS:
        c = _gap_case(W, g, corners)
        _contract(c)
        assert oracle.run_stages(pc.params(ElasParams, c.over), *_post_pair(c)) >= 3
        ch = _post_want(oracle, c)
        assert _same(ch["speckle1"], c.left), "speckle_size 0: the painted map reaches the stage as it is"
        G = ch["gap1"]
        assert not (c.left[0] >= 0).any() and (G != c.left).any()
        if W > 68:
            assert (G[2, 64:67] == 11).all() and (G[6, 63:66] == 10.5).all() and (G[8, 62:65] == 11).all()
            assert g == 3 or (G[10, 61:65] == 10).all()                      # (13 - 10 = 3 is no smooth step: the smaller end)
            assert g != 3 or corners or (G[10, 61:65] == pc.INV).all()
        if g == 3:
            assert (W < 101 or (G[12, 20:90] == pc.INV).all()) and (G[16, 0:3] == (12 if corners else pc.INV)).all() and (G[16, W - 3:] == (14 if corners else pc.INV)).all()
        else:
            assert (G[14, 3:W - 1] == 9.5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("W", GAP_W)
def test_gap_rows_against_the_oracle(eng, oracle, W):
    for g, corners in GAP_PARAMS:
        _run_post(eng, oracle, _gap_case(W, g, corners))


# ---- support matching ---------------------------------------------------------------------------------------------------------------------
SUP_W, SUP_H, SUP_D, SUP_B = 330, 70, 64, 20


def _support_params(cls, disp_min):
    p = cls.driver(SUP_D - 1)
    p.disp_min = disp_min
    return p


def _support_want(oracle, disp_min, i):
    def run():
        L, R = util.pkg("synth").make_pair(200 + i, SUP_H, SUP_W, SUP_D)
        p = _support_params(ElasParams, disp_min)
        n = oracle.run_stages(p, L, R)
        Wc, Hc = oracle.stage("dcan_dims")
        d1, d2, _ = oracle.process(p, L, R)
        return dict(L=L, R=R, n=np.array(n), dcan=oracle.stage("dcan_raw").reshape(Hc, Wc).copy(), d1=d1, d2=d2)
    return _once(("support", disp_min, i), run)


@pytest.mark.parametrize("disp_min", (0, 3))
def test_support_cases_have_clipped_and_whole_ranges(oracle, disp_min):
    w = _support_want(oracle, disp_min, 0)
    Hc, Wc = w["dcan"].shape
    assert (Wc, Hc) == (66, 14) and int(w["n"]) >= 3
    assert 2 * 13 * SUP_B > 512 and 2 * 13 <= 512, "the batch takes k_support<false, 4>, a pair alone the 8-wavefront one"
    # lattice columns below (5 + 63) / 5 have a range cut by the image border (per lane), the columns behind them have the whole range;
    # the second workgroup of a lattice row holds column 65 alone, which lies in the right border
    assert (w["dcan"][1:, 1:14] >= 0).any() and (w["dcan"][1:, 14:65] >= 0).any() and (w["dcan"][1:, 65] == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("disp_min", (0, 3))
def test_support_match_against_the_oracle(eng, oracle, disp_min):
    want = [_support_want(oracle, disp_min, i) for i in range(SUP_B)]
    # one pair alone on a keep_debug handle: the lattice itself
    e = eng.StereoEngine(SUP_W, SUP_H, _support_params(eng.SvParams, disp_min), keep_debug=True, n_workers=2)
    try:
        for w in want[:2]:
            _, _, status = e.process_host(w["L"], w["R"])
            assert int(status[0]) == int(w["n"]) and _same(e.debug("dcan_raw"), w["dcan"].ravel())
    finally:
        e.close()
    # twenty pairs in one chunk: every map the lattice leads to
    e = eng.StereoEngine(SUP_W, SUP_H, _support_params(eng.SvParams, disp_min), chunk=SUP_B, n_workers=2)
    try:
        assert e.query()["chunk"] == SUP_B
        d1, d2, status = e.process_host(np.stack([w["L"] for w in want]), np.stack([w["R"] for w in want]))
        for i, w in enumerate(want):
            assert int(status[i]) == int(w["n"]) and _same(d1[i], w["d1"]) and _same(d2[i], w["d2"]), i
    finally:
        e.close()
