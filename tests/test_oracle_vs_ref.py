"""CPU: the oracle restatement against the reference itself on inputs beyond the committed digests.json cases: seeded
synthetic and random inputs and the reference's bundled image pairs (committed under tests/golden/).  The reference's side
of every comparison: its results stored in tests/golden/ref_digests.json (sha256 of every stage, written from oracle/_ref by
make_golden.py --ref-digests over the case generators below) and, where oracle/_ref was built, the compiled reference itself."""
import json
import os
import sys

import numpy as np
import pytest

import content_cases
import degenerate_sets
import util
from pyoracle import ElasParams, RefElas

SYNTHETIC = [(11, 140, 400, 64), (12, 90, 333, 48), (13, 200, 640, 128), (14, 64, 128, 32)]
PRESETS = ["driver", "robotics", "middlebury"]
KITTI_MINI_FRAMES = range(21)
CONTENT_EARLY_STAGES = ["desc1", "desc2", "dcan_raw", "support"]  # what a pair with fewer than three support points produces
PROFILE_PAIRS = ["aloe", "cones", "raindeer", "urban1", "urban2", "urban3", "urban4"]


@pytest.fixture(scope="module")
def ref():
    """The compiled reference where oracle/_ref exists, else None (the stored digests alone)."""
    return RefElas() if RefElas.available() else None


@pytest.fixture(scope="module")
def stored():
    with open(os.path.join(util.GOLDEN, "ref_digests.json")) as f:
        return json.load(f)


def stage_digests(lib, p, L, R):
    """{"n": support points, "stages": {stage: sha256}} of one run of `lib` (the reference or the oracle)."""
    n = lib.run_stages(p, L, R)
    return {"n": n, "stages": {k: util.sha(lib.stage(k)) for k in util.STAGES}}


def _compare(ref, oracle, stored, key, p, L, R):
    got = stage_digests(oracle, p, L, R)
    want = stored[key]
    assert got["n"] == want["n"]
    bad = [k for k in util.STAGES if got["stages"][k] != want["stages"][k]]
    assert not bad, bad
    if ref is not None:
        assert ref.run_stages(p, L, R) == got["n"]
        bad = [k for k in util.STAGES if not np.array_equal(ref.stage(k).view(np.uint8), oracle.stage(k).view(np.uint8))]
        assert not bad, bad


def synthetic_case(seed, H, W, D, preset):
    L, R = util.pkg("synth").make_pair(seed, H, W, D)
    p = ElasParams.driver(D - 1) if preset == "driver" else ElasParams.preset(preset)
    p.disp_max = D - 1
    return "synthetic_%d_%dx%d_d%d_%s" % (seed, W, H, D, preset), p, L, R


def noise_cases():
    rng = np.random.default_rng(3)
    L = rng.integers(0, 256, (100, 260), dtype=np.uint8)
    R = np.roll(L, -7, axis=1)
    R[::3] = rng.integers(0, 256, R[::3].shape, dtype=np.uint8)
    for preset in ("robotics", "middlebury"):
        p = ElasParams.preset(preset)
        p.disp_max = 31
        yield "noise_%s" % preset, p, L, R


def textureless_cases():
    """(driver stages case, ROBOTICS Elas::process case): all-zero images."""
    L = np.zeros((80, 200), np.uint8)
    p = ElasParams.preset("robotics")
    p.disp_max = 63
    return ("textureless_driver", ElasParams.driver(63), L, L), ("textureless_robotics_maps", p, L, L)


def delaunay_sets():
    """(iteration, mode, n, xy float32) of the random point sets Triangle is fed."""
    rng = np.random.default_rng(0)
    for it in range(600):
        mode = it % 5
        n = int(rng.integers(3, 300)) if it % 10 else int(rng.integers(3, 10))
        if mode == 0:
            pts = rng.integers(0, 60, (n, 2)) * 5
        elif mode == 1:
            pts = np.stack([rng.integers(-50, 300, n), rng.integers(0, 75, n) * 5], 1)
        elif mode == 2:
            pts = rng.integers(0, 4000, (n, 2))
        elif mode == 3:
            pts = np.stack([rng.integers(0, 8, n) * 5, rng.integers(0, 8, n) * 5], 1)
        else:
            pts = np.stack([np.arange(n) * 5, (np.arange(n) % 3) * 5], 1)
        u = np.unique(pts, axis=0)
        if len(u) < 3:
            continue
        d = u - u[0]
        k = np.flatnonzero((d != 0).any(1))[0]
        if np.all(d[:, 0] * d[k, 1] == d[:, 1] * d[k, 0]):
            continue  # all collinear: Triangle yields no triangles; ELAS never feeds that
        yield it, mode, n, pts.astype(np.float32)


def random_parameter_cases():
    """(key, values, params, L, R) of the parameter sets far from the presets."""
    sys.path.insert(0, util.ROOT + "/tools")
    import fuzz_params as fz

    rng = np.random.default_rng(21)
    shapes = [(150, 260), (97, 203), (128, 401)]
    for i in range(15):
        vals = fz.random_params(rng)
        H, W = shapes[i % 3]
        L, R = util.pkg("synth").make_pair(500 + i, H, W, min(vals["disp_max"] + 1, 64))
        yield "random_parameters_%d" % i, vals, fz.apply(ElasParams.preset("robotics"), vals), L, R


def kitti_mini_case(frame):
    return "kitti_mini_%d_d128" % frame, ElasParams.driver(127), util.load_png("kitti%d_left.png" % frame), util.load_png("kitti%d_right.png" % frame)


def profile_case(name, preset):
    return ("profile_%s_%s" % (name, preset), ElasParams.preset(preset), util.load_png("profile_%s_left.png" % name),
            util.load_png("profile_%s_right.png" % name))


@pytest.mark.parametrize("seed,H,W,D", SYNTHETIC)
@pytest.mark.parametrize("preset", PRESETS)
def test_synthetic_pairs(ref, oracle, stored, seed, H, W, D, preset):
    _compare(ref, oracle, stored, *synthetic_case(seed, H, W, D, preset))


def test_noise_images(ref, oracle, stored):
    """Pure noise: few, scattered support points, many invalid pixels, heavy speckle removal."""
    for case in noise_cases():
        _compare(ref, oracle, stored, *case)


def test_textureless_images(ref, oracle, stored):
    """The reference's own smoke test feeds all-zero images (tests/test_demo.py:8-10): no lattice point passes the
    texture gate, the driver preset still triangulates its six corner points; ROBOTICS returns early."""
    driver, (key, p, L, _) = textureless_cases()
    _compare(ref, oracle, stored, *driver)
    D1o, D2o, _ = oracle.process(p, L, L)
    assert [util.sha(D1o), util.sha(D2o)] == stored[key] and not D1o.any()
    if ref is not None:
        D1r, D2r, _ = ref.process(p, L, L)
        assert np.array_equal(D1r, D1o) and np.array_equal(D2r, D2o) and not D1r.any()


def test_delaunay_random_sets(ref, oracle, stored):
    """Lattice points (co-circular quadruples everywhere), duplicates (right-image collisions), strips."""
    want = stored["delaunay_random_sets"]
    done = 0
    for it, mode, n, xy in delaunay_sets():
        b = oracle.delaunay(xy)
        assert [b.shape[0], util.sha(b)] == want[str(it)], (it, mode, n)
        if ref is not None:
            a = ref.delaunay(xy)
            assert a.shape == b.shape and np.array_equal(a, b), (it, mode, n)
        done += 1
    assert done > 400 and done == len(want)


def test_delaunay_structured_sets(ref, oracle, stored):
    """The structured sets of tests/degenerate_sets.py - wholly collinear sets (no triangle), collinear halves, fans, strips, complete
    lattices up to a 4K support grid, co-circular quadruples at the extremes of the coordinate box: the restatement's triangle list
    equals the reference's Triangle's.  No set is left out."""
    want = stored["delaunay_structured_sets"]
    done = empty = 0
    for name, xy in degenerate_sets.sets():
        b = oracle.delaunay(xy.astype(np.float32))
        assert [b.shape[0], util.sha(b)] == want[name], name
        if degenerate_sets.is_collinear(xy):
            assert b.shape[0] == 0, name
            empty += 1
        if ref is not None:
            a = ref.delaunay(xy.astype(np.float32))
            assert a.shape == b.shape and np.array_equal(a, b), name
        done += 1
    assert done == len(want) == 592 and empty == 100


def degenerate_pair_case(name):
    """(key, params, L, R, the reference can run it).  Images of at most 40 rows: the compiled reference does not survive them
    (tests/test_gpu_parity.py::test_small_and_odd_image_sizes); the memory-safe restatement defines the result, and the key says so."""
    L, R, _, _ = degenerate_sets.make_pair(name)
    by_ref = L.shape[0] > 40
    return ("degenerate_pair_" if by_ref else "oracle_defined_degenerate_pair_") + name, degenerate_sets.pair_params(ElasParams, name), L, R, by_ref


@pytest.mark.parametrize("name", [c[0] for c in degenerate_sets.pair_cases()])
def test_pairs_with_degenerate_support_sets(ref, oracle, stored, name):
    """ROBOTICS with add_corners = 0.  One textured band on one lattice row (column) of a flat image: three or more support points, all on
    one line in both images (in the left image only) - a triangulation without a triangle, and the pipeline carries on.  A complete support
    lattice; two lattice rows at the smallest admitted height.  Every stage of the restatement equals the reference's (for the 32-row pair,
    which the reference cannot run, the stored digests are the restatement's own: a regression record under a key that says so); the shape
    of the support set is what each case is for."""
    key, p, L, R, by_ref = degenerate_pair_case(name)
    kind = {c[0]: c[1] for c in degenerate_sets.pair_cases()}[name]
    _compare(ref if by_ref else None, oracle, stored, key, p, L, R)
    n, t1, t2 = stored[key]["n"], oracle.stage("tri1").size // 3, oracle.stage("tri2").size // 3
    sup = oracle.stage("support").reshape(-1, 3)
    us, vs = np.unique(sup[:, 0]), np.unique(sup[:, 1])
    assert n >= 3 and [t1, t2] == stored[key]["triangles"]
    if kind == "row":
        assert len(vs) == 1 and t1 == 0 and t2 == 0
    elif kind == "col":
        assert len(us) == 1 and t1 == 0 and t2 > 0
    elif kind == "lattice":
        assert n == len(us) * len(vs) and len(us) >= 8 and len(vs) >= 8 and t1 > 0 and t2 > 0
        assert (np.diff(us) == p.candidate_stepsize).all() and (np.diff(vs) == p.candidate_stepsize).all()
    else:
        assert L.shape[0] == 32 and len(vs) == 2 and vs[1] - vs[0] == p.candidate_stepsize and n >= 6 and t1 > 0 and t2 > 0


def content_case(key):
    """(digest key, params, L, R) of one of tests/content_cases.py.  The compiled reference runs every one of them."""
    _, preset, over, L, R = content_cases.make(key)
    return content_cases.digest_key(key), content_cases.params(ElasParams, preset, over), L, R


@pytest.mark.parametrize("key", content_cases.keys())
def test_content_cases(ref, oracle, stored, key):
    """Pairs whose content forces exact ties, saturated descriptor bytes and matches at the ends of the disparity range
    (tests/content_cases.py; what each family is for is asserted in tests/test_content_edges.py): the support count and every stage of the
    restatement equal the reference's.  A pair with fewer than three support points ends after the support stage in both (elas.cpp:63-69):
    there the stages up to the support list are compared."""
    dkey, p, L, R = content_case(key)
    want = stored[dkey]
    names = util.STAGES if want["n"] >= 3 else CONTENT_EARLY_STAGES
    assert sorted(want["stages"]) == sorted(names)
    n = oracle.run_stages(p, L, R)
    assert n == want["n"]
    bad = [k for k in names if util.sha(oracle.stage(k)) != want["stages"][k]]
    assert not bad, bad
    if ref is not None:
        assert ref.run_stages(p, L, R) == n
        bad = [k for k in names if not np.array_equal(ref.stage(k).view(np.uint8), oracle.stage(k).view(np.uint8))]
        assert not bad, bad


def test_random_parameter_sets(ref, oracle, stored):
    """Parameter sets far from the presets (lattice step, window sizes, grid size, prior, thresholds, gap / speckle limits,
    filter switches, half resolution): every stage of the restatement equals the reference's."""
    for key, vals, p, L, R in random_parameter_cases():
        want = stored[key]
        n2 = oracle.run_stages(p, L, R)
        assert n2 == want["n"], vals
        if ref is not None:
            assert ref.run_stages(p, L, R) == n2, vals
        if n2 < 3:
            continue
        bad = [k for k in util.STAGES if util.sha(oracle.stage(k)) != want["stages"][k]]
        assert not bad, (bad, vals)
        if ref is not None:
            bad = [k for k in util.STAGES if not np.array_equal(ref.stage(k).view(np.uint8), oracle.stage(k).view(np.uint8))]
            assert not bad, (bad, vals)


@pytest.mark.parametrize("frame", KITTI_MINI_FRAMES)
def test_every_kitti_mini_pair(ref, oracle, stored, frame):
    """All 21 pairs the reference ships under datasets/kitti_mini, D = 128, the driver's preset: every stage of the restatement
    equals the compiled reference's (DESIGN.md section 1(c) claims it).  Inputs: the committed gray fixtures
    tests/golden/kitti<frame>_{left,right}.png (make_golden.py's OpenCV-4.x BGR2GRAY of the colour frames)."""
    _compare(ref, oracle, stored, *kitti_mini_case(frame))


@pytest.mark.parametrize("name", PROFILE_PAIRS)
@pytest.mark.parametrize("preset", ["robotics", "middlebury"])
def test_every_bundled_profile_pair(ref, oracle, stored, name, preset):
    """The seven Middlebury / urban pairs of datasets/profile with both presets (disp_max 255, the presets' own value).  Inputs:
    the committed lossless copies tests/golden/profile_<name>_{left,right}.png."""
    _compare(ref, oracle, stored, *profile_case(name, preset))
