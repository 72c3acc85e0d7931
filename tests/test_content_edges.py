"""The disparity engine on image content that forces ties, saturation and matches at the ends of the range (tests/content_cases.py).

CPU part: every family does what it is for, shown on the oracle's stages and the inputs alone - conditions, not tolerances.  (That the
oracle equals the reference on these cases is tests/test_oracle_vs_ref.py::test_content_cases.)

GPU part: every stage of every case against the oracle with the lattice filters on the host and on the GPU, all cases of one shape and
parameter set as one chunk-4 batch with the pairs of fewer than three support points in between, three cases through a chunk-1 handle,
and the pairs with long seam triangles through the GPU triangulation paths.  Tolerance 0 throughout."""
import numpy as np
import pytest

import content_cases as cc
import util
from pyoracle import ElasParams

EARLY = ["desc1", "desc2", "dcan_raw", "support"]  # what a pair with fewer than three support points still produces
_ORACLE = {}  # key -> (support count, {stage: array}): no case goes through the oracle twice


def _oracle(oracle, key):
    if key not in _ORACLE:
        _, preset, over, L, R = cc.make(key)
        n = oracle.run_stages(cc.params(ElasParams, preset, over), L, R)
        _ORACLE[key] = (n, {k: oracle.stage(k) for k in (util.STAGES if n >= 3 else EARLY)})
    return _ORACLE[key]


def _desc(oracle, key):
    """The interior of both descriptor images, [H - 6, W - 6, 16] (outside it they are zero by definition)."""
    H, W = cc.spec(key)[3]
    st = _oracle(oracle, key)[1]
    return [st[k].reshape(H, W, 16)[3:H - 3, 3:W - 3] for k in ("desc1", "desc2")]


def _texture_sum(d):
    return np.abs(d.astype(np.int32) - 128).sum(-1)


# ---- CPU: each family does what it is for

def test_the_cases_are_what_the_issue_asks_for():
    keys = cc.keys()
    assert len(keys) == len(set(keys)) == 40
    widths = set()
    for key in keys:
        fam, preset, over, (H, W) = cc.spec(key)
        _, _, _, L, R = cc.make(key)
        assert L.shape == R.shape == (H, W) and 67 <= H <= 100 and 160 <= W <= 260 and 15 <= over["disp_max"] <= 63, key
        widths.add(W)
    assert any(w % 4 for w in widths)
    for fam in set(cc.FAMILY.values()) - {"noise"}:  # (noise_cases() has its own two presets)
        assert {cc.spec(k)[1] for k in cc.keys(fam)} == {"driver", "robotics"}, fam


@pytest.mark.parametrize("key", cc.keys("rowconst"))
def test_row_constant_pairs_tie_everywhere(oracle, key):
    """L = R = f(v): the interior of both descriptor images is constant along u, so every disparity has the same energy at every pixel.
    Measured: all 78 interior rows pass support_texture = 10 (vertical gradients only); no lattice point
    becomes a support point (a tie never passes the ratio test): 6 corner points under the driver preset, 0 under ROBOTICS."""
    _, preset, over, L, R = cc.make(key)
    assert np.array_equal(L[:, 1:], L[:, :-1]) and np.array_equal(L, R)
    d1, d2 = _desc(oracle, key)
    assert np.array_equal(d1[:, 1:], d1[:, :-1]) and np.array_equal(d1, d2)
    textured = int((_texture_sum(d1[:, 0]) >= 10).sum())
    n, st = _oracle(oracle, key)
    print(key, "interior rows past the texture gate:", textured, "of", d1.shape[0], "support points:", n)
    assert textured > d1.shape[0] // 2
    assert n == (6 if preset == "driver" else 0) and not (st["dcan_raw"] > 0).any()


PERIODIC_CANDIDATES = {"p16-d3-m15": 1, "p16-d3-m19": 2, "p16-d3-m18": 1, "p8-d5-m23": 3, "p4-d2-m15": 4, "p24-d5-m28": 1}


@pytest.mark.parametrize("key", cc.keys("periodic"))
def test_periodic_pairs_tie_at_every_period(oracle, key):
    """Tile of period p, R(u) = L(u + d0): both images and the interior of both descriptor images repeat exactly after p columns, and
    the right descriptors are the left ones d0 columns on - so d0, d0 + p, ... have exactly equal (zero) energy.  The number of them
    inside [0, disp_max] is 1, 2, 1, 3, 4, 1 in the order of PERIODIC_CANDIDATES; p16-d3-m19 has d0 + p = disp_max, p16-d3-m18 and
    p24-d5-m28 have d0 + p = disp_max + 1."""
    var = key.split("_")[1]
    p, d0, dm = [int(x[1:]) for x in var.split("-")]
    _, _, over, L, R = cc.make(key)
    W = L.shape[1]
    assert over["disp_max"] == dm and p in (4, 8, 16, 24)
    assert np.array_equal(L[:, p:], L[:, :-p]) and np.array_equal(R[:, p:], R[:, :-p]) and np.array_equal(R[:, :W - d0], L[:, d0:])
    d1, d2 = _desc(oracle, key)
    assert np.array_equal(d1[:, p:], d1[:, :-p]) and np.array_equal(d2[:, p:], d2[:, :-p])
    assert np.array_equal(d2[:, :d2.shape[1] - d0], d1[:, d0:])
    assert len(range(d0, dm + 1, p)) == PERIODIC_CANDIDATES[var]


def test_periodic_pairs_cover_the_range_end():
    ends = {int(v.split("-")[1][1:]) + int(v.split("-")[0][1:]) - int(v.split("-")[2][1:]) for v in PERIODIC_CANDIDATES}  # d0 + p - disp_max
    assert {0, 1} <= ends and set(PERIODIC_CANDIDATES.values()) >= {1, 2, 3}
    assert {k.split("_")[1] for k in cc.keys("periodic")} == set(PERIODIC_CANDIDATES)


# share of the interior bytes of desc1 equal to 0 / to 255, as the test measured them (it asserts that both occur and prints them)
BINARY_SHARES = {"block1": (0.2014, 0.2020), "block2": (0.2529, 0.2532), "block4": (0.1261, 0.1278), "checker4": (0.2508, 0.2508)}


@pytest.mark.parametrize("key", cc.keys("binary"))
def test_binary_pairs_saturate_the_descriptors(oracle, key):
    """0 / 255 images: the Sobel responses leave [-128, 127] in both directions, so desc1 holds bytes clipped to 0 and to 255."""
    _, _, _, L, R = cc.make(key)
    assert set(np.unique(L)) == {0, 255} and set(np.unique(R)) == {0, 255}
    d1, _ = _desc(oracle, key)
    lo, hi = float((d1 == 0).mean()), float((d1 == 255).mean())
    print(key, "share of interior desc1 bytes at 0: %.4f, at 255: %.4f" % (lo, hi))
    assert lo > 0 and hi > 0
    assert (round(lo, 4), round(hi, 4)) == BINARY_SHARES[key.split("_")[1]]


@pytest.mark.parametrize("key", cc.keys("constant"))
def test_constant_pairs_have_flat_descriptors(oracle, key):
    _, preset, _, L, R = cc.make(key)
    assert L.min() == L.max() == int(key.split("_")[1]) and np.array_equal(L, R)
    d1, d2 = _desc(oracle, key)
    assert (d1 == 128).all() and (d2 == 128).all()
    assert _oracle(oracle, key)[0] == (6 if preset == "driver" else 0)


@pytest.mark.parametrize("key", cc.keys("edge"))
def test_range_edge_pairs_match_where_they_should(oracle, key):
    """Blurred noise, R(u) = L(u + d), disp_max 31.  Measured, driver / ROBOTICS: d = 0: every valid pixel of wta1 is 0 (16434 / 7290);
    d = 31 = disp_max: 13062 / 11140 pixels of wta1 at 31; d = 32: none at 32, nothing above 31 (and 88 / 7 support points, all of them
    wrong); d = 5 with disp_min = 6: no support point below 6 (85 / 14 support points)."""
    var = key.split("_")[1]
    _, _, over, L, R = cc.make(key)
    d, dm, W = cc.EDGE_SHIFT[var], over["disp_max"], L.shape[1]
    assert np.array_equal(R[:, :W - d], L[:, d:])
    n, st = _oracle(oracle, key)
    w1, sup = st["wta1"], st["support"].reshape(-1, 3)
    print(key, "support points:", n, "valid in wta1:", int((w1 >= 0).sum()), "at the true shift:", int((w1 == d).sum()), "at disp_max:", int((w1 == dm).sum()))
    assert n >= 3 and w1.max() <= dm
    if var == "zero":
        assert (w1 >= 0).any() and (w1[w1 >= 0] == 0).all() and (sup[:, 2] == 0).all()
    elif var == "atmax":
        assert d == dm and (w1 == dm).sum() > 0 and (sup[:, 2] == dm).any()
    elif var == "pastmax":
        assert d == dm + 1 and (w1 == d).sum() == 0
    else:
        assert d == over["disp_min"] - 1 and (sup[:, 2] >= over["disp_min"]).all()


@pytest.mark.parametrize("key", cc.keys("unrelated"))
def test_unrelated_pairs_fail_the_left_right_check(oracle, key):
    """Independent textures, disp_max 63: the left/right check invalidates more matched pixels than it keeps, and speckle removal and gap
    interpolation both change the map.  Measured, driver / ROBOTICS: 19 / 208 support points, 15910 / 11990 pixels matched in wta1, lr1
    keeps 6776 / 4429 and removes 9134 / 7561, speckle removal changes 6131 / 4357 pixels, gap interpolation 16323 / 8."""
    n, st = _oracle(oracle, key)
    w1, lr1, sp1, g1 = st["wta1"], st["lr1"], st["speckle1"], st["gap1"]
    kept, removed = int((lr1 >= 0).sum()), int(((w1 >= 0) & (lr1 < 0)).sum())
    print(key, "support points:", n, "wta1 valid:", int((w1 >= 0).sum()), "lr1 keeps:", kept, "removes:", removed,
          "speckle changes:", int((sp1 != lr1).sum()), "gap changes:", int((g1 != sp1).sum()))
    assert n >= 3
    assert removed > kept
    assert (sp1 != lr1).any() and (g1 != sp1).any()


@pytest.mark.parametrize("key", cc.keys("mixed"))
def test_mixed_pairs_have_support_on_one_side_and_triangles_across(oracle, key):
    """A support point's matching window reaches five pixels from it (block centres at +-2, descriptor taps +-2 around those, Sobel +-1).
    No support point from matching has its whole window beyond the seam (the six corner points are the last six of the list), and at
    least one triangle of the left triangulation joins a vertex on the textured side to one wholly beyond the seam - a corner point.
    Measured (v-constant, v-rowconst, v-periodic, h-constant, h-rowconst, h-periodic): 40, 19, 25, 22, 27, 18 matched support points, the
    farthest of them on the seam's own lattice line (u = 100 / v = 40); 3, 3, 2, 3, 2, 8 of the 82, 41, 54, 48, 58, 40 triangles cross."""
    seam = key.split("_")[1][0]
    axis, at = (0, cc.SEAM_U) if seam == "v" else (1, cc.SEAM_V)
    n, st = _oracle(oracle, key)
    sup = st["support"].reshape(-1, 3)
    matched, tri = sup[:-6], st["tri1"].reshape(-1, 3)
    c = sup[:, axis][tri]
    across = int(((c.min(1) < at) & (c.max(1) - 5 >= at)).sum())
    print(key, "matched support points:", len(matched), "largest coordinate across the seam axis:", int(matched[:, axis].max()), "seam at", at,
          "triangles:", len(tri), "across the seam:", across)
    assert len(matched) >= 10 and (matched[:, axis] - 5 < at).all()
    assert across >= 1


@pytest.mark.parametrize("key", cc.keys("texture"))
def test_texture_gate_rows(oracle, key):
    """Lattice step 10: the descriptors at the lattice points of rows 10, 20, 30 sum to 9, of rows 40, 50, 60 to 10, of rows 70, 80, 90 to
    11, and support_texture is 10: the raw lattice holds no match on the first three rows and matches on the other six.  Measured, both
    presets: 0, 0, 0, 19, 19, 19, 19, 19, 19 matches on the lattice rows 1 .. 9 (of 21 lattice points a row); 14 / 8 support points."""
    _, _, over, L, R = cc.make(key)
    H, W = L.shape
    assert over["candidate_stepsize"] == 10 and cc.params(ElasParams, *cc.spec(key)[1:3]).support_texture == 10
    n, st = _oracle(oracle, key)
    d1 = st["desc1"].reshape(H, W, 16)
    for j in range(1, 10):
        sums = _texture_sum(d1[10 * j, 10:W - 3:10])
        assert (sums == (9 if j <= 3 else 10 if j <= 6 else 11)).all(), (j, sums)
    dcan = st["dcan_raw"].reshape(-(-H // 10), -(-W // 10))
    counts = [int((dcan[j, 1:] >= 0).sum()) for j in range(1, 10)]
    print(key, "matches per lattice row 1 .. 9:", counts, "support points:", n)
    assert counts[:3] == [0, 0, 0] and min(counts[3:]) > 0
    assert counts[3:6] == counts[6:9]  # at the threshold and above it: the same matches


def test_both_ends_of_the_too_few_support_exit(oracle):
    """Across all cases: pairs with fewer than three support points (the maps stay untouched) and pairs with a map that is at least
    20 % valid.  Measured: 6 and 32 of the 40."""
    few = [k for k in cc.keys() if _oracle(oracle, k)[0] < 3]
    full = [k for k in cc.keys() if _oracle(oracle, k)[0] >= 3 and (_oracle(oracle, k)[1]["final1"] >= 0).mean() >= 0.2]
    print("fewer than 3 support points:", few, "\nat least 20 % valid:", len(full))
    assert len(few) >= 3 and len(full) >= 10


# ---- GPU

@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return util.pkg("engine")


def _maps(oracle, key, fill1, fill2):
    """(support count, D1, D2) a caller sees who handed over maps filled with fill1 / fill2: untouched with fewer than three points."""
    n, st = _oracle(oracle, key)
    if n < 3:
        return n, fill1, fill2
    shape = fill1.shape
    return n, st["final1"].reshape(shape), st["final2"].reshape(shape)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("gpu_filter", [False, True])
@pytest.mark.parametrize("key", cc.keys())
def test_every_stage_matches_the_oracle(eng, oracle, key, gpu_filter):
    """One keep_debug run per case and filter placement: the first differing stage names the kernel.  (Of a pair with fewer than three
    support points the descriptors and the raw lattice are compared and the count, which is the status; the short list itself is
    compared in test_lattice_filter_edges.py.)"""
    _, preset, over, L, R = cc.make(key)
    n, want = _oracle(oracle, key)
    e = eng.StereoEngine(L.shape[1], L.shape[0], cc.params(eng.SvParams, preset, over), keep_debug=True, gpu_filter=gpu_filter)
    try:
        d1, d2, status = e.process_host(L, R)
        got = {}
        names = [k for k in want if n >= 3 or k != "support"]
        for k in names:
            try:
                got[k] = e.debug(k)
            except KeyError:
                pass
    finally:
        e.close()
    bad = []
    for k in names:  # (in pipeline order)
        g, o = got.get(k), want[k]
        if g is None or g.size != o.size or not _same(g, o):
            bad.append((k, int((g != o).sum()) if g is not None and g.size == o.size else -1))
    assert not bad, "%s: first differing stage %s (%d elements); all: %s" % (key, bad[0][0], bad[0][1], bad)
    assert int(status[0]) == n, (key, int(status[0]), n)
    zero = np.zeros(L.shape, np.float32)
    _, o1, o2 = _maps(oracle, key, zero, zero)
    assert _same(d1[0], o1) and _same(d2[0], o2), key


def _groups():
    """{name: keys} of the cases that one handle can take: same shape, preset and overrides."""
    out = {}
    for k in cc.keys():
        _, preset, over, (H, W) = cc.spec(k)
        name = "%dx%d_%s_%s" % (W, H, preset, "_".join("%s=%s" % kv for kv in sorted(over.items())))
        out.setdefault(name, []).append(k)
    return out


GROUPS = _groups()


def _interleaved(oracle, keys):
    """The keys with every pair of fewer than three support points between two ordinary ones (as far as there are ordinary ones),
    repeated to at least five pairs: more than one chunk of four, the last one ragged."""
    few = [k for k in keys if _oracle(oracle, k)[0] < 3]
    ordinary = [k for k in keys if k not in few]
    out = []
    for i, k in enumerate(ordinary):
        if i and few:
            out.append(few.pop(0))
        out.append(k)
    out = out[:-1] + few + out[-1:]  # (more of them than gaps: the rest before the last ordinary pair)
    while len(out) < 5:
        out = out + out
    return out


def test_the_batches_mix_both_kinds_of_pairs(oracle):
    """The largest ROBOTICS batch has its pairs of fewer than three support points between ordinary ones."""
    keys = max((v for g, v in GROUPS.items() if "robotics" in g), key=len)
    order = _interleaved(oracle, keys)
    few = [i for i, k in enumerate(order) if _oracle(oracle, k)[0] < 3]
    assert len(keys) >= 8 and len(few) >= 3 and set(order) == set(keys)
    assert all(0 < i < len(order) - 1 and _oracle(oracle, order[i - 1])[0] >= 3 and _oracle(oracle, order[i + 1])[0] >= 3 for i in few)


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_batches_of_one_shape(eng, oracle, group):
    """All cases of one shape and parameter set through a chunk-4, two-slot, three-worker handle in one process_host call, the maps
    pre-filled with a pattern: ordinary pairs equal the oracle, pairs of fewer than three support points leave their maps exactly as they
    were handed over (status < 3).  Then the reversed batch on the same handle: each pair gives the same bytes in both positions."""
    order = _interleaved(oracle, GROUPS[group])
    _, preset, over, (H, W) = cc.spec(order[0])
    B = len(order)
    pattern = ((np.arange(B * H * W, dtype=np.int64) * 7919) % 251 - 125).astype(np.float32).reshape(B, H, W)
    e = eng.StereoEngine(W, H, cc.params(eng.SvParams, preset, over), chunk=4, n_slots=2, n_workers=3)
    try:
        runs = []
        for seq in (order, order[::-1]):
            left, right = np.stack([cc.make(k)[3] for k in seq]), np.stack([cc.make(k)[4] for k in seq])
            d1, d2, status = e.process_host(left, right, d1=pattern.copy(), d2=(pattern + 1000).copy())
            runs.append((seq, d1, d2, status))
    finally:
        e.close()
    for seq, d1, d2, status in runs:
        for i, k in enumerate(seq):
            n, o1, o2 = _maps(oracle, k, pattern[i], pattern[i] + 1000)
            assert int(status[i]) == n, (group, k, i, int(status[i]), n)
            assert _same(d1[i], o1), (group, k, i, "D1", "untouched" if n < 3 else int((d1[i] != o1).sum()))
            assert _same(d2[i], o2), (group, k, i, "D2", "untouched" if n < 3 else int((d2[i] != o2).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["rowconst_a_driver", "periodic_p16-d3-m19_driver", "binary_block1_driver"])
def test_latency_path(eng, oracle, key):
    """One pair per call through a chunk-1 handle (the calling thread drives the pair itself)."""
    _, preset, over, L, R = cc.make(key)
    zero = np.zeros(L.shape, np.float32)
    n, o1, o2 = _maps(oracle, key, zero, zero)
    e = eng.StereoEngine(L.shape[1], L.shape[0], cc.params(eng.SvParams, preset, over), chunk=1, n_slots=1, n_streams=1, n_workers=2)
    try:
        d1, d2, status = e.process_host(L, R)
    finally:
        e.close()
    assert int(status[0]) == n
    assert _same(d1[0], o1), (key, "D1", int((d1[0] != o1).sum()))
    assert _same(d2[0], o2), (key, "D2", int((d2[0] != o2).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["gpu", "resident", "round3"])
@pytest.mark.parametrize("key", cc.keys("mixed") + ["edge_atmax_driver", "edge_atmax_robotics"])
def test_triangulation_paths(eng, oracle, monkeypatch, key, path):
    """Long triangles across the seam, corner points that coincide with each other, and support points at disp_max through the
    triangulation on the GPU: with the host pool ordering the vertices ("gpu", as test_pipeline_with_gpu_triangulation), with the support
    lists resident on the device and with the lists sent to the host ("resident" / "round3", as
    test_resident_and_round3_triangulation_paths_agree)."""
    _, preset, over, L, R = cc.make(key)
    zero = np.zeros(L.shape, np.float32)
    n, o1, o2 = _maps(oracle, key, zero, zero)
    opts = dict(n_slots=2, n_workers=3) if path == "gpu" else dict(n_slots=3, n_workers=1, resident=None if path == "resident" else False)
    e = eng.StereoEngine(L.shape[1], L.shape[0], cc.params(eng.SvParams, preset, over), chunk=4, n_streams=2, triangulation="gpu", **opts)
    try:
        q = e.query()
        assert q["gpu_triangulation"] == 1 and (path == "gpu" or q["resident"] == int(path == "resident")), q
        d1, d2, status = e.process_host(np.stack([L] * 5), np.stack([R] * 5))
    finally:
        e.close()
    assert n >= 3 and (status == n).all(), (key, status, n)
    for i in range(5):
        assert _same(d1[i], o1), (key, path, i, "D1", int((d1[i] != o1).sum()))
        assert _same(d2[i], o2), (key, path, i, "D2", int((d2[i] != o2).sum()))
