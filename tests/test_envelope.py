"""The engine at the edges of what sv_create admits (engine.cpp validate / fill_kparams).

CPU part: the validator's boundaries.  sv_create validates before it looks for a device, so an admitted configuration asked for
device 1023 ends in SV_ERR_NO_DEVICE (no GPU) or "device ordinal out of range" (fewer GPUs), a refused one in SV_ERR_ARG naming its limit.

GPU part: seeded synthetic pairs (and one KITTI pair) at those edges - disparity ranges across every mask-word count, ranges shorter
than the support matching's split, plane radii up to 15, lattice steps and grids at both ends, the largest images, the dense stage's
float-division fallback and the lattice filter's limits - both maps bit for bit and the support count against the oracle, through a
chunk-4 batch and through the single-pair path.  Every case also asserts that it reached the code it is there for."""
import ctypes
import sys

import numpy as np
import pytest

import util
from pyoracle import ElasParams

SV_OK, SV_ERR_ARG, SV_ERR_NO_DEVICE = 0, -1, -3
SV_Q_GPU_LATTICE_FILTER = 3
LDS_PER_WORKGROUP = 160 * 1024
FILTER_MAX_LATTICE = 8192 * 256  # RSV_MAX_BLOCKS classify blocks of FCL_THREADS lattice points (kernels.hip)


# ---- restatements of the host-side decisions the cases steer

def support_lds_bytes(step, disp_max, split):
    """kernels.hip support_lds_bytes plus k_support's static 64-word texture table."""
    span = 63 * step
    return 2 * 64 * split * 8 + 16 * 2 * ((span + disp_max + 11) + (span + 2 * disp_max + 11)) + 4 * 64


def cell_mul(width, height, grid_size):
    """fill_kparams: the multiply-shift of k_dense's grid cell, or 0 where it (or the float quotient) misses u // grid_size for some
    column or row - then k_dense divides in float for the whole image."""
    m = (65536 + grid_size - 1) // grid_size
    if not (m < (1 << 24) and width <= 65536 and height <= 65536):
        return 0
    u = np.arange(max(width, height), dtype=np.uint64)
    want = u // np.uint64(grid_size)
    shift = ((u * np.uint64(m)) & np.uint64(0xFFFFFFFF)) >> np.uint64(16)
    flt = np.floor(u.astype(np.float32) / np.float32(grid_size)).astype(np.uint64)
    return m if bool(np.all(shift == want) and np.all(flt == want)) else 0


def params(cls, disp_max, preset="driver", **kw):
    p = cls.driver(disp_max) if preset == "driver" else cls.preset(preset)
    p.disp_max = disp_max
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---- CPU: the validator at each boundary

@pytest.fixture(scope="module")
def eng_lib():
    return util.pkg("engine")


def _create(eng, p, width, height):
    """(admitted, message) of sv_create for device 1023, which no machine has: nothing is allocated either way."""
    L = eng.lib()
    cfg = eng.SvConfig(width, height, 1023, 1, 1, 0, 1, 1)
    h = ctypes.c_void_p()
    rc = L.sv_create(ctypes.byref(p), ctypes.byref(cfg), ctypes.byref(h))
    msg = L.sv_last_error(None).decode()
    assert not h.value and rc != SV_OK, (rc, msg)
    admitted = rc == SV_ERR_NO_DEVICE or (rc == SV_ERR_ARG and msg == "device ordinal out of range")
    assert admitted or rc == SV_ERR_ARG, (rc, msg)
    return admitted, msg


def test_no_device_or_unknown_ordinal_after_validation(eng_lib):
    """What the other boundary tests rely on: an admitted configuration gets past validate() to the device lookup."""
    admitted, msg = _create(eng_lib, params(eng_lib.SvParams, 63), 320, 120)
    assert admitted, msg


@pytest.mark.parametrize("disp_max,ok", [(9, False), (10, True), (1023, True), (1024, False)])
def test_validate_disp_max(eng_lib, disp_max, ok):
    admitted, msg = _create(eng_lib, params(eng_lib.SvParams, disp_max), 320, 120)
    assert admitted == ok and (ok or "disp_max" in msg), msg


@pytest.mark.parametrize("width,height,ok", [(31, 32, False), (32, 31, False), (32, 32, True), (8192, 4096, True), (8193, 32, False),
                                             (32, 4097, False), (8192, 4097, False), (8193, 4096, False)])
def test_validate_image_size(eng_lib, width, height, ok):
    admitted, msg = _create(eng_lib, params(eng_lib.SvParams, 63), width, height)
    assert admitted == ok and (ok or "image size" in msg), msg


@pytest.mark.parametrize("sigma,sradius,ok", [(3.0, 5.0, True), (1.0, 15.0, True), (3.0, 5.0001, False), (1.0, 15.001, False), (5.0, 3.0, True)])
def test_validate_plane_radius(eng_lib, sigma, sradius, ok):
    assert (np.ceil(np.float32(sigma) * np.float32(sradius)) <= 15) == ok
    admitted, msg = _create(eng_lib, params(eng_lib.SvParams, 63, sigma=sigma, sradius=sradius), 320, 120)
    assert admitted == ok and (ok or "plane radius" in msg), msg


@pytest.mark.parametrize("disp_max,step,sub,ok", [(1023, 15, 0, True), (1023, 16, 0, False), (63, 37, 0, True), (63, 38, 0, False),
                                                  (63, 37, 1, False), (63, 36, 1, True), (10, 39, 0, True), (10, 40, 0, False)])
def test_validate_support_lds(eng_lib, disp_max, step, sub, ok):
    """Support matching stages two rows of both images around 64 lattice points: sv_create refuses what the batched (4-wavefront)
    launch cannot fit in a workgroup's 160 KiB; half resolution rounds the step up to even first."""
    eff = step + (step % 2 if sub else 0)
    assert (support_lds_bytes(eff, disp_max, 4) <= LDS_PER_WORKGROUP) == ok
    admitted, msg = _create(eng_lib, params(eng_lib.SvParams, disp_max, candidate_stepsize=step, subsampling=sub), 640, 480)
    assert admitted == ok, msg
    if not ok:
        assert "LDS" in msg and "candidate_stepsize %d" % eff in msg, msg


def test_validate_lattice_and_grid_lower_bounds(eng_lib):
    for kw in (dict(candidate_stepsize=0), dict(grid_size=0), dict(incon_window_size=-1)):
        admitted, msg = _create(eng_lib, params(eng_lib.SvParams, 63, **kw), 320, 120)
        assert not admitted and "lattice" in msg, (kw, msg)
    for kw in (dict(candidate_stepsize=1), dict(grid_size=1), dict(grid_size=100000), dict(incon_window_size=0), dict(disp_min=-50), dict(disp_min=2000)):
        admitted, msg = _create(eng_lib, params(eng_lib.SvParams, 63, **kw), 320, 120)
        assert admitted, (kw, msg)


def test_restated_checks_match_the_issue_numbers():
    """The restatements the GPU cases lean on: where cell_mul first drops to 0, and where a lone pair's 8-wavefront launch no longer fits."""
    assert cell_mul(4699, 40, 25) and not cell_mul(4700, 40, 25) and not cell_mul(8192, 40, 25)
    assert cell_mul(40, 2262, 31) and not cell_mul(40, 2263, 31) and not cell_mul(40, 4096, 31)
    assert cell_mul(1115, 375, 62) and not cell_mul(1242, 375, 62)
    assert all(cell_mul(8192, 4096, g) for g in (1, 2, 10, 16, 20, 32))
    assert support_lds_bytes(15, 1023, 4) <= LDS_PER_WORKGROUP < support_lds_bytes(15, 1023, 8)
    assert support_lds_bytes(5, 1023, 8) <= LDS_PER_WORKGROUP


# ---- GPU: maps against the oracle

@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return util.pkg("engine")


_ORACLE = {}  # (input key, parameter values) -> (support count, D1, D2): no input goes through the oracle twice


def _pvals(p):
    return tuple(getattr(p, f) for f, _ in ElasParams._fields_)


def _pair(key):
    if key[0] == "kitti":
        return util.load_png("kitti%d_left.png" % key[1]), util.load_png("kitti%d_right.png" % key[1])
    _, seed, H, W, D = key
    return util.pkg("synth").make_pair(seed, H, W, D)


def _oracle(oracle, key, po, L, R):
    ck = (key, _pvals(po))
    if ck not in _ORACLE:
        n = oracle.run_stages(po, L, R)
        Hm, Wm = (L.shape[0] // 2, L.shape[1] // 2) if po.subsampling else L.shape
        o1 = np.zeros((Hm, Wm), np.float32)
        o2 = np.zeros((Hm, Wm), np.float32)
        if n >= 3:  # (fewer: the maps stay as the caller handed them over, elas.cpp:63-69 - zeros here)
            o1, o2 = oracle.stage("final1").reshape(Hm, Wm), oracle.stage("final2").reshape(Hm, Wm)
        _ORACLE[ck] = (n, o1, o2)
    return _ORACLE[ck]


def _check(eng, oracle, keys, kw, modes=("batch", "single"), gpu_filter=None, expect_filter=None, min_valid=0.2, min_support=3, preset="driver"):
    """keys: the inputs ((kind, ...) tuples), kw: ElasParams fields on top of `preset`.  "batch" runs the inputs, repeated to four
    pairs, as one chunk-4 batch; "single" runs the first input alone (chunk 1: the lone-pair support launch).  Returns the handles' queries."""
    pe = params(eng.SvParams, kw["disp_max"], preset, **{k: v for k, v in kw.items() if k != "disp_max"})
    po = params(ElasParams, kw["disp_max"], preset, **{k: v for k, v in kw.items() if k != "disp_max"})
    pairs = [_pair(k) for k in keys]
    H, W = pairs[0][0].shape
    want = [_oracle(oracle, k, po, L, R) for k, (L, R) in zip(keys, pairs)]
    for n, o1, _ in want:  # the case is past the "too few points" exit and has a map to compare
        assert n >= min_support, (keys, kw, n)
        assert (o1 >= 0).mean() >= min_valid, (keys, kw, (o1 >= 0).mean())
    queries = []
    for mode in modes:
        if mode == "batch":
            idx = [i % len(pairs) for i in range(4 if W * H <= (1 << 21) else 2)]
            opts = dict(chunk=4, n_slots=2, n_streams=2, n_workers=4)
        else:
            idx = [0]
            opts = dict(chunk=1, n_slots=1, n_streams=1, n_workers=2)
        e = eng.StereoEngine(W, H, pe, gpu_filter=gpu_filter, **opts)
        try:
            q = e.query()
            d1, d2, status = e.process_host(np.stack([pairs[i][0] for i in idx]), np.stack([pairs[i][1] for i in idx]))
        finally:
            e.close()
        if expect_filter is not None:
            assert q["gpu_lattice_filter"] == expect_filter, (mode, keys, kw, q)
        queries.append(q)
        for j, i in enumerate(idx):
            n, o1, o2 = want[i]
            assert status[j] == n, (mode, keys[i], kw, int(status[j]), n)
            assert np.array_equal(d1[j].view(np.uint8), o1.view(np.uint8)), (mode, keys[i], kw, "D1", int((d1[j] != o1).sum()))
            assert np.array_equal(d2[j].view(np.uint8), o2.view(np.uint8)), (mode, keys[i], kw, "D2", int((d2[j] != o2).sum()))
    return queries


def _synth(seeds, H, W, D):
    return [("synth", s, H, W, D) for s in seeds]


@pytest.mark.gpu
@pytest.mark.parametrize("disp_max", [10, 31, 32, 255, 256, 512, 767, 1023])
def test_disparity_range(eng, oracle, disp_max):
    """Every mask-word count of the dense stage's candidate masks (MW = 1, 2, 8, 9, 16, 24, 32) and the generic kernel beyond its
    eight register words; disp_max 10 is also a range the 4- and 8-way support splits do not divide."""
    W = 1100 if disp_max > 300 else 400
    _check(eng, oracle, _synth((11, 12), 64, W, disp_max + 1), dict(disp_max=disp_max))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(40, 8192), (90, 600)])
def test_disparity_1023_wide_and_narrow(eng, oracle, shape):
    """disp_max 1023 on a strip far wider than the range (staged rows clipped on neither side) and on one narrower than it."""
    H, W = shape
    _check(eng, oracle, _synth((21,), H, W, min(1024, W)), dict(disp_max=1023))


@pytest.mark.gpu
def test_lone_pair_support_launch_falls_back_to_four_waves(eng, oracle):
    """candidate_stepsize 15 with disp_max 1023: admitted (it fits at four wavefronts per point), but a lone pair's eight-wavefront
    launch would need more than 160 KiB - it takes the four-wavefront kernel instead of failing."""
    assert support_lds_bytes(15, 1023, 4) <= LDS_PER_WORKGROUP < support_lds_bytes(15, 1023, 8)
    _check(eng, oracle, _synth((31,), 120, 1100, 1024), dict(disp_max=1023, candidate_stepsize=15), min_support=3)


@pytest.mark.gpu
@pytest.mark.parametrize("disp_min", [50, 52, 53, 57, 60, 62, 63, 64, 90])
def test_disp_min_against_the_range(eng, oracle, disp_min):
    """disp_max 63: support ranges of 14, 12 and 11 disparities (not multiples of either split: the last wavefronts' shares are short
    or empty), then 7 ... 1, an empty and a negative range (no point can match: only the corners remain)."""
    keys = _synth((41, 42), 96, 300, 64)
    _check(eng, oracle, keys, dict(disp_max=63, disp_min=disp_min))
    if disp_min <= 53:  # the matching itself produced support points, not just the four corners
        assert _ORACLE[(keys[0], _pvals(params(ElasParams, 63, disp_min=disp_min)))][0] > 50


@pytest.mark.gpu
@pytest.mark.parametrize("sradius,radius", [(14 / 3, 14), (4.5, 14), (5.0, 15), (13 / 3, 13)])
@pytest.mark.parametrize("disp_max", [10, 31, 1023])
def test_plane_radius(eng, oracle, sradius, radius, disp_max):
    """Plane radii 13 ... 15 (sigma 3): with disp_max 10 / 31 the band is wider than the whole range (one mask word), with 1023 it
    sits beside 32 words; the synthetic planes lie at d = 2 and near disp_max, so the band clips at d = 0 and d = D - 1."""
    assert int(max(np.ceil(np.float32(3.0) * np.float32(sradius)), 2)) == radius
    W = 1100 if disp_max > 300 else 300
    _check(eng, oracle, _synth((51,), 96, W, disp_max + 1), dict(disp_max=disp_max, sigma=3.0, sradius=sradius), modes=("batch", "single") if disp_max != 1023 else ("batch",))


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 2, 15, 16])
def test_lattice_step(eng, oracle, step):
    _check(eng, oracle, _synth((61, 62), 96, 200, 64), dict(disp_max=63, candidate_stepsize=step))


@pytest.mark.gpu
@pytest.mark.parametrize("step", [31, 32, 33])
def test_lattice_step_at_the_smallest_image(eng, oracle, step):
    """32 x 32: step 31 leaves one lattice point to match, 32 and more none (the lattice is cleared instead of matched)."""
    _check(eng, oracle, _synth((71,), 32, 32, 16), dict(disp_max=15, candidate_stepsize=step), min_valid=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("grid_size", [1, 2, 500])
def test_grid_size(eng, oracle, grid_size):
    """Grid cells of one and two pixels, and one cell larger than the whole image."""
    _check(eng, oracle, _synth((81, 82), 96, 300, 64), dict(disp_max=63, grid_size=grid_size))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(33, 8191), (4095, 33)])
def test_subsampling_odd_extremes(eng, oracle, shape):
    """Half resolution with odd widths and heights at the largest sizes: maps of (H // 2) x (W // 2)."""
    H, W = shape
    _check(eng, oracle, _synth((91,), H, W, 24), dict(disp_max=20, subsampling=1), min_valid=0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,disp_max,grid_size", [((40, 8192), 63, 25), ((4096, 40), 15, 31), ((40, 8192), 1023, 20), ((4096, 40), 15, 20)])
def test_image_strips_and_dense_fallback(eng, oracle, shape, disp_max, grid_size):
    """8192 x 40 and 40 x 4096 strips.  Grid 25 on the wide strip (first wrong column 4699) and grid 31 on the tall one (first wrong
    row 2262) take k_dense's float division; grid 20 keeps the multiply-shift."""
    H, W = shape
    want_mul = grid_size == 20
    assert (cell_mul(W, H, grid_size) != 0) == want_mul
    _check(eng, oracle, _synth((101,), H, W, min(disp_max + 1, W)), dict(disp_max=disp_max, grid_size=grid_size))


@pytest.mark.gpu
def test_dense_fallback_on_kitti(eng, oracle):
    """A real 1242 x 375 KITTI pair with grid 62: the multiply-shift is wrong from column 1115, so the whole image divides in float."""
    assert cell_mul(1242, 375, 62) == 0
    _check(eng, oracle, [("kitti", 0)], dict(disp_max=127, grid_size=62))


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("min_support,on_gpu", [(60, 1), (61, 0)])
def test_lattice_filter_limits(eng, oracle, step, min_support, on_gpu):
    """window 5 (11 x 11, 120 neighbours), threshold 4095, min_support 60: the largest the GPU filter takes (6-bit late counts);
    61 sends the same filters to the host."""
    _check(eng, oracle, _synth((111, 112), 96, 200, 64), dict(disp_max=63, candidate_stepsize=step, incon_window_size=5, incon_threshold=4095,
                                                               incon_min_support=min_support), modes=("batch",), gpu_filter=True, expect_filter=on_gpu)


@pytest.mark.gpu
def test_lattice_beyond_the_filter_block_table(eng, oracle):
    """2048 x 1100 at step 1: 2 252 800 lattice points, more than the GPU filter's resolve step orders (2 097 152) - the handle keeps the
    filters on the host even when asked for the GPU, and the maps equal the oracle's."""
    assert 2048 * 1100 > FILTER_MAX_LATTICE
    _check(eng, oracle, _synth((121,), 1100, 2048, 64), dict(disp_max=63, candidate_stepsize=1), modes=("batch",), gpu_filter=True, expect_filter=0)


@pytest.mark.gpu
def test_largest_image(eng, oracle):
    """One 8192 x 4096 pair, driver preset, disp_max 63: lattice filters on the GPU and on the host, one oracle run for both."""
    keys = _synth((131,), 4096, 8192, 64)
    assert (8192 // 5 + 1) * (4096 // 5 + 1) <= FILTER_MAX_LATTICE
    for gpu_filter in (True, False):
        _check(eng, oracle, keys, dict(disp_max=63), modes=("single",), gpu_filter=gpu_filter, expect_filter=int(gpu_filter))


@pytest.mark.gpu
def test_random_parameters_across_the_envelope(eng, oracle):
    """tools/fuzz_params.py's wide draws (disp_max to 1023, steps 1 ... 16, grids 1 ... 64, radii to 15, disp_min past disp_max):
    both maps, batch and single-pair paths, bit-exact."""
    sys.path.insert(0, util.ROOT + "/tools")
    import fuzz_params as fz

    rng = np.random.default_rng(77)
    shapes = [(150, 260), (97, 203), (128, 401)]
    for i in range(9):
        vals = fz.random_params(rng, wide=True)
        res = fz.run_case(util.pkg("engine"), oracle, util.pkg("synth"), vals, 900 + i, shapes[i % 3])
        assert all(r[0] and r[1] for r in res), (res, vals)
