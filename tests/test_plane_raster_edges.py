"""The middle block of the disparity engine - k_grid_mark, k_grid_dilate, k_planes with solve3, k_raster_tiles and the plane-dependent half
of k_dense in csrc/kernels.hip - on the support lattices of tests/plane_raster_cases.py, which are painted point by point: plane slopes
on both sides of the 0.7 validity test, disparity folds that reverse the right image's corner order, right-image columns left of the
image, sets of three and of six points, lattice rows on a raster-tile seam, tile lists below, at and above their cap, disparities at the
ends of the mask words for every mask width, clusters the flat dilation wraps into the next cell row, half resolution.

CPU: the constants the cases restate are the source's; every case keeps the lattice contract and is what it says; the cases' numpy
restatement of grid, validity and scan conversion equals the oracle (orc_grid, orc_planes, orc_raster) on every case and differs from
it under every mistake the case names; wta is -10 exactly where tri_id is -1 (or the column lies in findMatch's margin).
GPU: every case injected into keep_debug handles with the lattice filters on the GPU and on the host, and support, tri, planes, grid,
tri_id and wta of both sides compared with the oracle's chain byte for byte - the tile-list cases with every cap."""
import os
import re
import time

import numpy as np
import pytest

import plane_raster_cases as pc
import util
from pyoracle import ElasParams

KERNELS = os.path.join(util.ROOT, util.PKG, "csrc", "kernels.hip")
CHAIN = ("support", "tri1", "tri2", "planes1", "planes2", "grid1", "grid2", "tri_id1", "tri_id2", "wta1", "wta2")
SEED, SEED_D = 11, 24   # the one synthetic pair per image size
_WANT = {}


def _pair(c):
    return util.pkg("synth").make_pair(SEED, c.H, c.W, SEED_D)


def _want(oracle, c):
    """The oracle's chain for a case on the seeded pair of its size: computed once, shared, left unchanged."""
    if c.name not in _WANT:
        L, R = _pair(c)
        ch = oracle.chain_from_lattice(pc.params(ElasParams, c), c.lattice, L, R)
        for a in ch.values():
            a.setflags(write=False)
        _WANT[c.name] = ch
    return _WANT[c.name]


def _same(a, b):
    return a.size == b.size and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_the_constants_are_the_sources():
    src = open(KERNELS).read()
    for name, val in (("RT_W", pc.RT_W), ("RT_H", pc.RT_H), ("RT_CAP", pc.RT_CAP), ("DENSE_MASK_WORDS", pc.MASK_WORDS)):
        assert re.search(r"#define %s (\d+)" % name, src).group(1) == str(val), name
    raster = src[src.index("void k_raster_tiles("):src.index("void launch_triangles(")]
    assert "threadIdx.x & %d" % (pc.LANES - 1) in raster and "base += %d" % pc.LANES in raster and "u >= r.b_u" in raster
    planes = src[src.index("void k_planes("):src.index("void k_raster_tiles(")]
    assert "(double)fabsf(plane_a) < %s && (double)fabsf(plane_d) < %s" % (pc.VALID, pc.VALID) in planes
    assert "max((int)vlo - 1, 0)" in planes and "min((int)vhi + 2, d.H)" in planes and "max(r.a_u, 0)" in planes and "min(r.c_u, d.W)" in planes
    assert "c >= d.gw + 1 && c <= d.ncell - d.gw - 2" in src   # the flat dilation's range
    assert {ElasParams.driver().grid_size, ElasParams.preset("robotics").grid_size} == {pc.GRID}


def test_the_cases_keep_the_contract():
    assert sorted(pc.FAMILIES) == sorted(["slopes", "folds", "negative", "sparse", "seams", "tiles", "words", "dilation", "subsampling"])
    named = set()
    for c in pc.CASES.values():
        d = c.lattice
        assert d.dtype == np.int16 and d.min() >= -1 and d.max() <= c.disp_max and not d[0].any() and not d[:, 0].any(), c.name
        assert c.W <= 320 and c.H <= 170 and c.aim and c.over["incon_min_support"] == 0, c.name
        assert c.bugs and set(c.bugs) <= set(pc.BUGS), c.name
        named |= set(c.bugs)
    assert named == set(pc.BUGS)
    words = [pc.CASES[n] for n in pc.FAMILIES["words"]]
    assert sorted({(c.disp_max + 32) // 32 for c in words}) == [2, 3, 4, 6, 8, 9] and 9 > pc.MASK_WORDS   # the compiled widths, the generic one, past the register words
    assert {c.preset for c in words} == {"driver", "robotics"}
    assert {pc.params(ElasParams, c).match_texture for c in words} == {0, 1}
    assert {(c.W, c.H) for c in (pc.CASES[n] for n in pc.FAMILIES["seams"])} == {(320, 170), (64, 32), (65, 33)}
    assert sum(c.sub for c in pc.CASES.values()) == 2


def _tri_columns(sup, tri, right):
    """Per triangle (a_u, b_u, c_u) and whether the corner sort swapped."""
    out = []
    for t in tri:
        A, B, C, swapped = pc.corners(sup, t, right)
        out.append((int(A[0]), int(B[0]), int(C[0]), swapped))
    return np.array(out, np.int64).reshape(-1, 4)


def _check_aim(oracle, c):
    ch, x = _want(oracle, c), c.expect
    sup = ch["support"]
    assert _same(sup, c.painted()), "the oracle's list is not the painted set"
    if "n" in x:
        assert len(sup) == x["n"]
    if len(sup) < 3:
        return
    cols = [_tri_columns(sup, ch["tri%d" % s], s - 1) for s in (1, 2)]
    # a left-image triangle of lattice points has a vertical edge: (int)A_u == (int)B_u or (int)B_u == (int)C_u
    if not c.add_corners and c.family not in ("sparse", "dilation", "seams"):
        assert ((cols[0][:, 0] == cols[0][:, 1]) | (cols[0][:, 1] == cols[0][:, 2])).all()
    if "nt" in x:
        assert (len(ch["tri1"]), len(ch["tri2"])) == x["nt"]
    if "t1a" in x:
        for pl in (ch["planes1"], ch["planes2"]):   # (an exact zero comes out of the double elimination as a residue of 1e-16 times the offset)
            assert (pl[:, 0] == np.float32(x["t1a"])).all() if x["t1a"] else (np.abs(pl[:, 0]) < 1e-12).all(), np.abs(pl[:, 0]).max()
    if "valid" in x:
        for s in (1, 2):
            v = pc.valid(ch["planes%d" % s], s - 1)
            assert v.all() if x["valid"][s - 1] else not v.any(), (s, int(v.sum()), len(v))
    if c.name == "slope_m07":   # valid only because the float is compared in double
        assert not pc.valid(ch["planes1"], 0, "float_valid").any()
    if c.name == "slope_m08":   # invalid on the right by plane_d alone: its own slope is -0.8 / 1.8
        assert (np.abs(ch["planes2"][:, 3]) < 0.5).all() and (np.abs(ch["planes2"][:, 0]) > pc.VALID).all()
    if c.name == "slope_p05":   # invalid on the left by plane_d alone
        assert (ch["planes1"][:, 0] == 0.5).all() and (ch["planes1"][:, 3] == 1.0).all()
    if c.name == "slope_p04":
        assert (np.abs(ch["planes1"][:, 3] - 2 / 3) < 1e-6).all()
    if x.get("folds"):
        assert not _same(ch["tri1"], ch["tri2"]), "the fold must change the right image's triangulation"
        a, b, cc, swapped = cols[1].T
        assert swapped.any() and (x["folds"] == "swap" or ((a == b).any() and (b == cc).any())), (int(swapped.sum()), int((a == b).sum()), int((b == cc).sum()))
        right_u = sup[:, 0] - sup[:, 2]
        row = sup[:, 1] == sup[0, 1]
        assert (np.diff(right_u[row][np.argsort(sup[row, 0])]) < 0).any(), "u - d must fall somewhere along a row"
    if x.get("negative"):
        right_u = sup[:, 0] - sup[:, 2]
        assert ((right_u > -pc.GRID) & (right_u < 0)).any(), "a point that is no grid cell under floor and cell 0 under truncation"
        a, b, cc, _ = cols[1].T
        assert (cc <= 0).any() and ((a < 0) & (cc > 0)).any(), "right-image triangles left of column 0 and across it"
    if "far_left" in x:
        assert (sup[:, 0] - sup[:, 2]).min() <= x["far_left"]
    if x.get("big"):
        for s in (1, 2):
            info = {}
            pc.scan(sup, ch["tri%d" % s], c.W, c.H, s - 1, info=info)
            b = info["boxes"]
            assert ((b[:, 1] - b[:, 0] >= 2 * pc.RT_W) & (b[:, 3] - b[:, 2] >= 2 * pc.RT_H)).any() and info["trips"] >= 25, (s, info["trips"])
    if x.get("singular"):   # corners on one line in the other image: the reference divides by the elimination's residue
        _, singular = pc.planes(sup, ch["tri2"])
        assert singular[:, 0].any() and (np.abs(ch["planes2"][singular[:, 0], 0]) > 1e12).any()
    if x.get("seam"):
        assert (sup[:, 1] == 5 * pc.RT_H).sum() >= 30 and {60, 65} <= set(sup[:, 0].tolist()) and pc.RT_W - 4 == 60
    if "values" in x:
        assert sorted(set(sup[:, 2].tolist())) == x["values"] and {0, 1, 31, 32, 33, 63, c.disp_max - 1, c.disp_max} <= set(x["values"])
    if "wrap" in x:
        lo, hi = x["wrap"]
        g = ch["grid1"]
        own = lambda cell: [int(v) for v in cell[1:1 + cell[0]] if lo <= v <= hi]
        assert all((s[0] // pc.GRID == g.shape[1] - 1) == (lo < s[2] < hi) for s in sup), "the cluster, and nothing else, lies in the last grid column"
        # the cluster's cells are (1, last) and (2, last): flat neighbours of column 0 of the rows 2, 3 and 4 (cell (1, 0) lies in front of the range)
        assert own(g[2, 0]) and own(g[3, 0]) and own(g[4, 0]), "the last column's cluster must show in column 0 of the rows below"
        assert not g[1, 0].any() and not own(g[2, 1]) and not own(g[3, 2]) and own(g[2, -1]) and own(g[2, -2])
    if x.get("end_rows"):
        for s in (1, 2):
            g = ch["grid%d" % s]
            assert not g[0].any() and not g[-1].any() and g[1, :, 0].any() and g[-2, :, 0].any()
        assert (sup[:, 1] < pc.GRID).sum() == 3 and (sup[:, 1] >= c.H - pc.GRID).sum() == 3
    if x.get("empty_grid"):
        assert ch["grid1"].shape[:2] == (2, 2) and not ch["grid1"].any() and not ch["grid2"].any()
    if c.family == "tiles":
        cnt = [pc.tile_counts(pc.footprints(sup, ch["tri%d" % s], c.W, c.H, s - 1), c.W, c.H) for s in (1, 2)]
        if x.get("over_cap"):
            assert cnt[0].max() > pc.RT_CAP and cnt[1].max() > pc.RT_CAP and cnt[0].min() <= pc.RT_CAP, (cnt[0].max(), cnt[1].max())
        for cap in _caps(oracle, c):
            if cap is not None and cap > 1:
                assert any((k < cap).any() and (k == cap).any() and (k > cap).any() for k in cnt), (cap, cnt)
    if c.sub:
        assert ch["tri_id1"].shape == (c.H, c.W) and ch["wta1"].shape == (c.H // 2, c.W // 2)


def _caps(oracle, c):
    """The rt_cap values of a case: None (the handle's own 512), and for "tile" the count of one tile of the left image's map such that
    tiles below, at and above it exist."""
    ch = _want(oracle, c)
    out = [None]
    for cap in c.rt_caps:
        if cap == "tile":
            cnt = np.sort(np.unique(pc.tile_counts(pc.footprints(ch["support"], ch["tri1"], c.W, c.H, 0), c.W, c.H)))
            assert len(cnt) >= 3
            cap = int(cnt[len(cnt) // 2])
        out.append(cap)
    return out


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_the_cases_are_what_they_say(oracle, family):
    for name in pc.FAMILIES[family]:
        try:
            _check_aim(oracle, pc.CASES[name])
        except AssertionError as err:
            raise AssertionError("%s: %s" % (name, err))


_PART = dict(b_exclusive="scan", first_wins="scan", row_inclusive="scan", tile_clip="scan", floor_edge="scan", float_valid="valid", same_side_d="valid", le_valid="valid",
             row_dilation="grid", trunc_cell="grid", no_clamp="grid")


def _restated(c, ch, part, side, bug=None, info=None):
    sup = ch["support"]
    if part == "scan":
        return pc.scan(sup, ch["tri%d" % side], c.W, c.H, side - 1, bug, info)
    if part == "grid":
        return pc.grid(sup, c.W, c.H, c.disp_max, side - 1, bug)
    return pc.valid(ch["planes%d" % side], side - 1, bug)


def _oracle_part(ch, part, side):
    if part == "valid":   # elas.cpp:910 on orc_planes' floats, written out
        pl = ch["planes%d" % side]
        a, d = (pl[:, 0], pl[:, 3]) if side == 1 else (pl[:, 3], pl[:, 0])
        return np.array([abs(float(p)) < 0.7 and abs(float(q)) < 0.7 for p, q in zip(a, d)], bool)
    return ch[{"scan": "tri_id%d", "grid": "grid%d"}[part] % side]


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_the_restatement_is_the_oracle_and_the_mistakes_show(oracle, family):
    """Grid, validity and scan conversion of plane_raster_cases equal orc_grid, orc_planes' validity and orc_raster on both sides of
    every case; the plane fit by Cramer's rule equals orc_planes within one unit in the last place of the float (and 1e-9 for the
    residue the Gauss-Jordan steps leave of an exact zero in double) wherever the system is regular; no row outside the image is asked for before the clip; k_planes'
    binning footprint holds every pixel a triangle writes.  Under every mistake the case names, the part that makes it differs from the
    oracle on one side at least; under the two silent ones nothing differs."""
    for name in pc.FAMILIES[family]:
        c = pc.CASES[name]
        ch = _want(oracle, c)
        if len(ch["support"]) < 3:
            continue
        for side in (1, 2):
            info = {}
            assert np.array_equal(_restated(c, ch, "scan", side, info=info), ch["tri_id%d" % side]), (name, side, "scan")
            assert info["outside"] == 0, (name, side)
            fp, b = pc.footprints(ch["support"], ch["tri%d" % side], c.W, c.H, side - 1), info["boxes"]
            drawn = b[:, 0] >= 0
            assert (b[drawn, 0] >= fp[drawn, 0]).all() and (b[drawn, 1] < fp[drawn, 1]).all() and (b[drawn, 2] >= fp[drawn, 2]).all() and (b[drawn, 3] < fp[drawn, 3]).all(), (name, side)
            assert np.array_equal(_restated(c, ch, "grid", side), ch["grid%d" % side]), (name, side, "grid")
            assert np.array_equal(_restated(c, ch, "valid", side), _oracle_part(ch, "valid", side)), (name, side, "valid")
            mine, singular = pc.planes(ch["support"], ch["tri%d" % side])
            regular = np.repeat(~singular, 3, axis=1)
            assert not singular[:, side - 1].any() and np.allclose(mine[regular], ch["planes%d" % side][regular], rtol=2.0 ** -23, atol=1e-9), (name, side, "planes")
        for bug in c.bugs:
            part = _PART[bug]
            assert any(not np.array_equal(_restated(c, ch, part, side, bug), _oracle_part(ch, part, side)) for side in (1, 2)), (name, bug)
        for bug in pc.SILENT:
            part = _PART[bug]
            assert all(np.array_equal(_restated(c, ch, part, side, bug), _oracle_part(ch, part, side)) for side in (1, 2)), (name, bug)


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_wta_is_set_where_a_triangle_covers(oracle, family):
    """At full resolution and without a texture test, orc_dense leaves -10 exactly where orc_raster leaves -1 or the column lies in
    findMatch's margin of two: the scan conversion as a stage of its own is the loop the dense stage walks."""
    done = 0
    for name in pc.FAMILIES[family]:
        c = pc.CASES[name]
        ch = _want(oracle, c)
        if c.sub or pc.params(ElasParams, c).match_texture > 0 or len(ch["support"]) < 3:
            continue
        u = np.arange(c.W)
        margin = (u < 2) | (u >= c.W - 2)
        for side in (1, 2):
            assert np.array_equal(ch["wta%d" % side] == -10, (ch["tri_id%d" % side] == -1) | margin[None, :]), (name, side)
        done += 1
    assert done or family in ("subsampling",)


def test_run_stages_keeps_the_scan_conversion(oracle):
    """orc_run_stages puts tri_id1 / tri_id2, and the chain from its own lattice is its own stages."""
    c = pc.CASES["slope_m06"]
    L, R = _pair(c)
    p = ElasParams.driver(63)
    n = oracle.run_stages(p, L, R)
    assert n >= 3
    own = {k: oracle.stage(k).copy() for k in CHAIN + ("dcan_raw",)}
    Wc, Hc = oracle.stage("dcan_dims")
    ch = oracle.chain_from_lattice(p, own["dcan_raw"].reshape(Hc, Wc), L, R)
    for k in CHAIN:
        assert _same(ch[k].ravel(), own[k]), k
    assert own["tri_id1"].size == c.W * c.H and own["tri_id1"].max() == len(ch["tri1"]) - 1


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    util.pkg("build").build()
    return util.pkg("engine")


_GROUPS = {}
for _c in pc.CASES.values():
    _GROUPS.setdefault(_c.key(), []).append(_c.name)
_GROUP_KEYS = sorted(_GROUPS, key=repr)


@pytest.mark.gpu
@pytest.mark.parametrize("g", range(len(_GROUP_KEYS)), ids=lambda g: _GROUPS[_GROUP_KEYS[g]][0])
def test_injected_lattices_against_the_oracle(eng, oracle, g):
    """Two keep_debug handles per (image size, parameters), lattice filters on the GPU and on the host.  Every case of the group is
    injected and run on the seeded pair of its size - the tile-list cases once per cap - and the support list, both triangulations,
    planes, grids, tri_id and wta of both sides are the oracle's chain, byte for byte; the status is the list's length.  The hook is
    cleared at the end, after which the pair is itself again."""
    t0 = time.time()
    names = _GROUPS[_GROUP_KEYS[g]]
    c0 = pc.CASES[names[0]]
    L, R = _pair(c0)
    handles = [eng.StereoEngine(c0.W, c0.H, pc.params(eng.SvParams, c0), keep_debug=True, gpu_filter=on, n_workers=2) for on in (True, False)]
    runs = 0
    try:
        assert [e.query()["gpu_lattice_filter"] for e in handles] == [1, 0]
        for name in names:
            c = pc.CASES[name]
            want = _want(oracle, c)
            for e in handles:
                e.debug_inject("lattice", np.array(c.lattice))
                for cap in _caps(oracle, c):
                    e.debug_set("rt_cap", -1 if cap is None else cap)
                    _, _, status = e.process_host(L, R)
                    assert int(status[0]) == len(want["support"]), (name, cap, status)
                    assert _same(e.debug("dcan_raw"), c.lattice.ravel()), (name, "dcan_raw is not the painted lattice")
                    bad = [k for k in CHAIN if k in want and not _same(e.debug(k), want[k].ravel())]
                    assert not bad, (name, cap, bad)
                    runs += 1
                e.debug_set("rt_cap", -1)
        n_own = oracle.run_stages(pc.params(ElasParams, c0), L, R)
        own = {k: oracle.stage(k).copy() for k in ("support", "tri_id1", "wta2")} if n_own >= 3 else {"support": oracle.stage("support").copy()}
        for e in handles:
            e.debug_inject("lattice", None, None)
            _, _, status = e.process_host(L, R)
            assert int(status[0]) == n_own and all(_same(e.debug(k), own[k]) for k in own), (names, "after the hook is cleared")
    finally:
        for e in handles:
            e.close()
    print("%s: %d cases, %d runs on 2 handles, %.2f s" % (names[0], len(names), runs, time.time() - t0))
