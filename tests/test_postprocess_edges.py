"""The second half of the disparity engine - L/R check (k_lr, k_lr2), speckle removal (k_ccl_band / border / total / apply and the
per-pixel ccl_legacy_map), gap interpolation (k_gap_rows, k_gap_cols), adaptive mean (k_amean, k_amean_sub) and median (k_median) - on the
maps of tests/postprocess_cases.py, which are painted pixel by pixel and handed to the engine through sv_debug_inject.  Every stage behind
the injection and the returned maps are compared with the oracle's single stages (postprocess_cases.chain) byte for byte; there is no
tolerance anywhere.

CPU: chain() against the oracle's own pipeline on uninjected pairs; every family's cases against what they are aimed at (measured with the
cases module's own labelling and on the oracle's output); what of sv_debug_inject's refusals needs no handle.
GPU: one test per case, cases of one shape and parameter set on one handle in turn (consecutive pairs on one slot are part of what is
tested); a table overflow, a clean pair and another overflow on one handle; the refusals on live handles.

One-token mutations of csrc/kernels.hip that these tests were run against on an MI355X (none is committed), and the tests that fail:
  `>=` -> `>` in k_ccl_band's CCL_LARGE line       size_one_band, size_two_bands, links_stacked, topo_arms, similar_*, words_4100, ... (12)
  `<= gw` -> `< gw` in k_gap_rows                  gap_rows_g3_c0 .. g7_c1, noise_*, filt_*_half (9)
  `nv - pv - 1` -> `nv - pv` in k_gap_cols         gap_cols_*, gap_interplay, words_127, words_130, ... (15)
  `< 3.0f` -> `<= 3.0f` in gap_value               gap_rows_*, gap_cols_*, table_k, ... (16)
  `> thr` -> `>= thr` in k_lr2                     lr_even_64, lr_even_130_t1, lr_half_130
  TOT[root] `>=` -> `>` in k_ccl_apply             size_two_bands, size_three_bands, links_stairs, ... (14)
  `<` -> `<=` in ccl_legacy_map's last loop        table_k_plus_1, table_last_band, noise_65x64_cap, test_overflow_then_clean_then_overflow
  carry from the valid mask, not the link mask     links_stacked, sides_different (k_ccl_band's carry and k_ccl_border's alike)
Three more change no map, so no test of outputs can fail for them: `| carry` dropped in ccl_new_links (an extra union of two runs that
are linked anyway), `r.y >= speckle_size` -> `>` in k_ccl_apply (a run of that length belongs to a band-local component of at least
that size, whose records k_ccl_band has pointed at CCL_LARGE), `T > cap` -> `T >= cap` (the map goes the per-pixel way and gives the
same bits)."""
import ctypes
import time

import numpy as np
import pytest

import postprocess_cases as pc
import util
from pyoracle import ElasParams


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


_PAIRS, _CHAINS = {}, {}


def _pair(shape):
    """The image pair that carries the cases of one image shape."""
    if shape not in _PAIRS:
        _PAIRS[shape] = util.pkg("synth").make_pair(pc.PAIR_SEED, shape[0], shape[1], pc.PAIR_D)
    return _PAIRS[shape]


def _chain(oracle, name):
    """The reference stages of a case, computed once and left unchanged."""
    if name not in _CHAINS:
        c = pc.CASES[name]
        out = pc.chain(oracle, pc.params(ElasParams, c.over), c.stage, c.left, c.right)
        for m in out.values():
            m.setflags(write=False)
        _CHAINS[name] = out
    return _CHAINS[name]


# ---- CPU: the reference chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, over", [((120, 320), {}), ((120, 320), dict(subsampling=1)), ((84, 202), dict(postprocess_only_left=1, filter_median=0, add_corners=1)),
                                         ((121, 323), dict(subsampling=1, postprocess_only_left=1, filter_adaptive_mean=0, speckle_size=40, ipol_gap_width=7))])
def test_chain_is_the_oracles_own_pipeline(oracle, shape, over):
    """chain(the oracle's wta1, wta2) == the oracle's lr ... final stages of an uninjected pair, byte for byte, at full and half resolution."""
    p = pc.params(ElasParams, dict(over, disp_max=63))
    L, R = util.pkg("synth").make_pair(7, shape[0], shape[1], 64)  # (the carrier pairs of the cases are too small to leave much of a map)
    assert oracle.run_stages(p, L, R) >= 3
    Hm, Wm = (shape[0] // 2, shape[1] // 2) if p.subsampling else shape
    want = {s + side: oracle.stage(s + side, (Hm, Wm)) for s in ("wta",) + pc.STAGES for side in "12"}
    got = pc.chain(oracle, p, "wta", want["wta1"], want["wta2"])
    for a, b in (("wta", "lr"), ("lr", "speckle"), ("speckle", "gap"), ("gap", "final")):
        assert (want[a + "1"] != want[b + "1"]).any(), "the stage %s changes nothing on this pair" % b
    for s in pc.STAGES:
        for side in "12":
            assert _same(got[s + side], want[s + side]), (s + side, int((got[s + side] != want[s + side]).sum()))
    again = pc.chain(oracle, p, "lr", want["lr1"], want["lr2"])
    assert all(_same(again[k], got[k]) for k in got)


def test_the_carrier_pairs_pass_the_support_stage(oracle):
    """Every image shape and parameter set of the cases: three or more support points, so that the injected maps are used."""
    seen = set()
    for c in pc.CASES.values():
        key = c.handle_key()
        if key in seen:
            continue
        seen.add(key)
        L, R = _pair(c.image_shape)
        assert oracle.run_stages(pc.params(ElasParams, c.over), L, R) >= 3, c.name


def test_the_cases_keep_the_contract_of_the_hook():
    """Injected values are ones the engine itself can produce: "lr" -10 or an integer in 0 .. disp_max, "wta" also -1."""
    for c in pc.CASES.values():
        for m in (c.left, c.right):
            ok = ((m >= 0) & (m <= pc.DISP_MAX) & (m == np.floor(m))) | (m == -10) | ((m == -1) if c.stage == "wta" else False)
            assert ok.all(), (c.name, m[~ok][:5])
        assert c.map_shape[1] in (64, 65, 127, 129, 130, 4100) and c.map_shape[0] in (33, 65, 67), c.name
        assert c.expect, c.name
    assert sorted(pc.FAMILIES) == sorted(["size", "words", "links", "topology", "similarity", "tables", "speckle_noise", "sides", "gaps", "lr", "filters"])


def _check(case, ch, labels, x):
    """One entry of a case's `expect` (see postprocess_cases)."""
    p = pc.params(ElasParams, case.over)
    thr = p.speckle_sim_threshold
    kind = x[0]

    def lab(side):
        if side not in labels:
            labels[side] = pc.components(case.maps(side), thr)
        return labels[side]

    if kind == "comp":
        _, side, (v, u), size, kept = x
        label, sizes = lab(side)
        assert case.maps(side)[v, u] >= 0 and sizes[label[v, u]] == size, (x, sizes.get(label[v, u]))
        s_eff = int(np.sqrt(np.float32(p.speckle_size)) * 2) if p.subsampling else p.speckle_size
        assert kept == (size >= s_eff), x
        out = ch["speckle%d" % (side + 1)][v, u]
        assert (out == case.maps(side)[v, u]) if kept else (out == -10), (x, out)
    elif kind == "run":
        _, side, v, u0, u1 = x
        D = case.maps(side)
        st = pc.run_starts(D, thr)
        assert (D[v, u0:u1 + 1] >= 0).all() and st[v, u0] and not st[v, u0 + 1:u1 + 1].any(), x
        assert u1 == D.shape[1] - 1 or D[v, u1 + 1] < 0 or st[v, u1 + 1], x
    elif kind == "runs":
        _, side, band, n = x
        assert int(pc.run_starts(case.maps(side), thr)[8 * band:8 * band + 8].sum()) == n, x
    elif kind == "total_runs":
        assert int(pc.run_starts(case.maps(x[1]), thr).sum()) == x[2], x
    elif kind == "path":
        _, side, (v, u), size = x
        label, sizes = lab(side)
        assert sizes[label[v, u]] == size and len(sizes) == 1 and pc.neighbours(case.maps(side), thr).max() == 2, x
        assert (case.maps(side) >= 0).any(axis=1).all(), "the path passes through every row, so through every band"
    elif kind == "at":
        _, stage, side, (v, u), val = x
        assert ch["%s%d" % (stage, side + 1)][v, u] == val, (x, ch["%s%d" % (stage, side + 1)][v, u])
    elif kind in ("same", "changed"):
        _, stage, side, (v, u) = x
        same = kind == "same" or (stage == "amean" and not p.filter_adaptive_mean)  # (a stage that is switched off changes nothing)
        assert (ch["%s%d" % (stage, side + 1)][v, u] == case.maps(side)[v, u]) == same, x
    elif kind == "median":
        v, u = x[1]
        assert ch["final1"][v, u] == (-10 if p.filter_median else ch["amean1"][v, u]) and ch["amean1"][v, u] >= 0, x
    elif kind == "differs":
        assert (ch[x[1] + "1"] != ch[x[2] + "1"]).any(), x
    elif kind == "corners":
        _, T, l1, l2, l3, g, Ln = x
        G = ch["gap1"].T if T else ch["gap1"]
        fill = bool(p.add_corners)
        assert (G[l1, 0:g] == (12 if fill else -10)).all(), x                        # open at the start by g: all of it, or nothing
        assert G[l2, 0] == -10 and (G[l2, 1:g + 1] == (12 if fill else -10)).all(), x  # ... by g + 1: the first pixel stays
        assert (G[l2, Ln - g:Ln] == (14 if fill else -10)).all(), x                   # open at the end by g
        assert G[l3, Ln - 1] == -10 and (G[l3, Ln - 1 - g:Ln - 1] == (14 if fill else -10)).all(), x
    elif kind == "both":
        valid = case.left >= 0
        wiped = valid & (ch["speckle1"] < 0)
        assert wiped.any() and (valid & ~wiped).any(), x
    else:
        raise AssertionError("unknown expectation %r" % (x,))


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_the_cases_realise_what_they_are_aimed_at(oracle, family):
    """Every expectation of every case of the family, on the injected maps and on the oracle's output."""
    for name in pc.FAMILIES[family]:
        case, labels = pc.CASES[name], {}
        for x in case.expect:
            try:
                _check(case, _chain(oracle, name), labels, x)
            except AssertionError as err:
                raise AssertionError("%s: %s" % (name, err))


def test_families_cover_both_outcomes(oracle):
    """Speckle families remove and keep components; the gap cases fill and leave gaps; the L/R cases keep and remove on both sides."""
    for fam in ("size", "words", "links", "topology", "similarity", "tables", "sides"):
        kept = [x[4] for n in pc.FAMILIES[fam] for x in pc.CASES[n].expect if x[0] == "comp"]
        assert True in kept and False in kept, fam
    for n in pc.FAMILIES["gaps"]:
        vals = [x[4] for x in pc.CASES[n].expect if x[0] == "at"]
        assert any(v >= 0 for v in vals) and (any(v < 0 for v in vals) or n == "gap_4100_corners"), n  # (g = 5000 with corners fills the whole map)
    for n in pc.FAMILIES["lr"]:
        for side in (0, 1):
            vals = [x[4] for x in pc.CASES[n].expect if x[0] == "at" and x[2] == side]
            assert sum(v >= 0 for v in vals) >= 3 and sum(v < 0 for v in vals) >= 5, n
    # the record pool: 4096 runs fit it, 4097 do not, no band of either overflows its table (at most 8 x 65 runs)
    for n in (4096, 4097):
        st = pc.run_starts(pc.CASES["table_pool_%d" % n].left, 1.0)
        assert st.sum() == n and max(int(st[b:b + 8].sum()) for b in range(0, 67, 8)) <= 520
    assert max(130 * 67 // 4, 4096) == 4096


def test_inject_needs_a_handle():
    """Without a handle the hook refuses with a text; the wrapper refuses maps of the wrong size or type before the library sees them."""
    util.pkg("build").build()
    eng = util.pkg("engine")
    L = eng.lib()
    L.sv_debug_inject.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    L.sv_debug_inject.restype = ctypes.c_int
    m = np.zeros((33, 64), np.float32)
    assert L.sv_debug_inject(None, b"lr", m.ctypes.data, m.ctypes.data) == -1 and L.sv_last_error(None).startswith(b"sv_debug_inject")
    e = eng.StereoEngine.__new__(eng.StereoEngine)  # (no device here: the size check comes before the handle is touched)
    e.map_height, e.map_width, e._h = 33, 64, None
    for bad in (np.zeros((33, 65), np.float32), np.zeros((32, 64), np.float32), np.zeros((33, 64), np.float64), np.zeros(33 * 64, np.float32), [[0.0] * 64] * 33):
        with pytest.raises(ValueError):
            e.debug_inject("lr", bad, m)
        with pytest.raises(ValueError):
            e.debug_inject("lr", m, bad)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    util.pkg("build").build()
    return util.pkg("engine")


class _Handles:
    """The handle of the cases that run now; cases arrive sorted by handle key, so that each handle is made once."""

    def __init__(self, eng):
        self.eng, self.key, self.e = eng, None, None
        self.count, self.seconds, self.made = {}, {}, 0

    def get(self, case):
        key = case.handle_key()
        if key != self.key:
            self.close()
            H, W = case.image_shape
            self.e = self.eng.StereoEngine(W, H, pc.params(self.eng.SvParams, case.over), keep_debug=True, n_workers=2)
            self.key, self.made = key, self.made + 1
        return self.e

    def close(self):
        if self.e is not None:
            try:
                self.e.debug_inject("lr", None, None)
            finally:
                self.e.close()
                self.e = self.key = None


@pytest.fixture(scope="module")
def handles(eng):
    h = _Handles(eng)
    try:
        yield h
    finally:
        h.close()
        print("\npainted-map cases per family (cases, seconds on the GPU side): " +
              ", ".join("%s %d %.2f" % (f, h.count[f], h.seconds[f]) for f in sorted(h.count)) +
              "; %d cases on %d handles, %.2f s" % (sum(h.count.values()), h.made, sum(h.seconds.values())))


def _run(e, oracle, name):
    """Injects the case, processes the carrier pair once and compares every stage behind the injection and the returned maps."""
    case = pc.CASES[name]
    want = _chain(oracle, name)
    L, R = _pair(case.image_shape)
    e.debug_set("ccl_cap", case.ccl_cap)
    e.debug_inject(case.stage, case.left, case.right)
    d1, d2, status = e.process_host(L, R)
    assert int(status[0]) >= 3, (name, status)
    got = {s + side: e.debug(s + side).reshape(case.map_shape) for s in pc.STAGES + (("wta",) if case.stage == "wta" else ()) for side in "12"}
    if case.stage == "wta":
        assert _same(got["wta1"], case.left) and _same(got["wta2"], case.right), (name, "the wta snapshot is not what was injected")
    bad = [(k, int((got[k] != want[k]).sum()), [tuple(int(i) for i in q) for q in np.argwhere(got[k] != want[k])[:4]])
           for s in pc.STAGES for k in (s + "1", s + "2") if not _same(got[k], want[k])]
    assert not bad, "%s: first differing stage %s (%d pixels, first at %s); all: %s" % (name, bad[0][0], bad[0][1], bad[0][2], [b[:2] for b in bad])
    assert _same(d1[0], want["final1"]), (name, "d1", int((d1[0] != want["final1"]).sum()))
    assert _same(d2[0], want["final2"]), (name, "d2", int((d2[0] != want["final2"]).sum()))


_ORDER = sorted(pc.CASES, key=lambda n: (repr(pc.CASES[n].handle_key()), list(pc.CASES).index(n)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", _ORDER)
def test_painted_map(handles, oracle, name):
    """One case: the stages lr, speckle, gap, amean and final of both sides and the returned maps equal the oracle's, byte for byte."""
    case = pc.CASES[name]
    _chain(oracle, name)
    t0 = time.perf_counter()
    try:
        _run(handles.get(case), oracle, name)
    finally:
        handles.count[case.family] = handles.count.get(case.family, 0) + 1
        handles.seconds[case.family] = handles.seconds.get(case.family, 0.0) + time.perf_counter() - t0


@pytest.mark.gpu
def test_overflow_then_clean_then_overflow(eng, oracle):
    """One slot, five pairs: a band over its run table (the map takes the per-pixel path and leaves its mark), a map that fits, the record
    pool overflowing without the hook, a map that fits, the last band alone over its table.  A mark that outlived its pair would send a
    clean map the slow way or keep an overflowing one on the fast one; either way the bits are the oracle's."""
    seq = [("table_k_plus_1", pc.A), ("table_k", pc.A), ("table_last_band", pc.A), ("table_k", pc.A), ("table_k_plus_1", pc.A)]
    e = eng.StereoEngine(pc.A[1], pc.A[0], pc.params(eng.SvParams, {}), keep_debug=True, n_workers=2)
    try:
        for name, _ in seq:
            _run(e, oracle, name)
        e.debug_inject("lr", None, None)
    finally:
        e.close()
    e = eng.StereoEngine(pc.B[1], pc.B[0], pc.params(eng.SvParams, {}), keep_debug=True, n_workers=2)
    try:
        for name in ("table_pool_4097", "table_pool_4096", "topo_spiral", "table_pool_4097", "table_pool_4096"):
            _run(e, oracle, name)
        e.debug_inject("lr", None, None)
    finally:
        e.close()


@pytest.mark.gpu
def test_cleared_injection_and_snapshots(eng, oracle):
    """After the hook is cleared the handle computes the pair's own maps again, and an injected "lr" map is what the lr snapshot returns."""
    case = pc.CASES["size_one_run"]
    L, R = _pair(case.image_shape)
    p = pc.params(ElasParams, case.over)
    assert oracle.run_stages(p, L, R) >= 3
    own = {k: oracle.stage(k, case.map_shape) for k in ("wta1", "lr1", "lr2", "final1", "final2")}
    e = eng.StereoEngine(L.shape[1], L.shape[0], pc.params(eng.SvParams, case.over), keep_debug=True, n_workers=2)
    try:
        e.debug_inject("lr", case.left, case.right)
        e.process_host(L, R)
        assert _same(e.debug("lr1").reshape(case.map_shape), case.left) and _same(e.debug("lr2").reshape(case.map_shape), case.right)
        assert _same(e.debug("wta1").reshape(case.map_shape), own["wta1"])
        e.debug_inject("lr", None, None)
        d1, d2, _ = e.process_host(L, R)
        assert _same(e.debug("lr1").reshape(case.map_shape), own["lr1"]) and _same(d1[0], own["final1"]) and _same(d2[0], own["final2"])
    finally:
        e.close()


@pytest.mark.gpu
def test_inject_refusals(eng):
    """No keep_debug, an unknown stage, one map missing, values outside the contract: SV_ERR_ARG and a text, and nothing is staged."""
    H, W = 33, 64
    ok = np.full((H, W), -10, np.float32)
    e = eng.StereoEngine(W, H, pc.params(eng.SvParams, {}), n_workers=2)
    try:
        with pytest.raises(eng.StereoError, match="keep_debug"):
            e.debug_inject("lr", ok, ok)
        with pytest.raises(eng.StereoError, match="keep_debug"):
            e.debug_inject("lr", None, None)
    finally:
        e.close()
    e = eng.StereoEngine(W, H, pc.params(eng.SvParams, {}), keep_debug=True, n_workers=2)
    try:
        with pytest.raises(eng.StereoError, match="unknown stage"):
            e.debug_inject("speckle", ok, ok)
        with pytest.raises(ValueError):
            e.debug_inject("lr", np.zeros((H, W + 1), np.float32), ok)
        L = eng.lib()
        assert L.sv_debug_inject(e._h, b"lr", ok.ctypes.data, None) == -1 and b"both maps" in L.sv_last_error(e._h)
        for stage, bad in (("lr", -1.0), ("lr", 0.5), ("lr", pc.DISP_MAX + 1.0), ("lr", -9.0), ("lr", float("nan")), ("lr", float("inf")), ("wta", -2.0),
                           ("wta", 3.25), ("wta", pc.DISP_MAX + 1.0), ("wta", -10.5)):
            for side in (0, 1):
                m = ok.copy()
                m[H - 1, W - 1] = bad
                with pytest.raises(eng.StereoError, match="sv_debug_inject"):
                    e.debug_inject(stage, *((ok, m) if side else (m, ok)))
        for stage, fine in (("lr", 0.0), ("lr", float(pc.DISP_MAX)), ("wta", -1.0), ("wta", -10.0), ("wta", float(pc.DISP_MAX))):
            m = ok.copy()
            m[0, 0] = fine
            e.debug_inject(stage, m, m)
        e.debug_inject("wta", None, None)
    finally:
        e.close()
