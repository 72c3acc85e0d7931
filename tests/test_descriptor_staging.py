"""GPU (MI355X): the descriptor staging of the matching kernels (expand_quad in csrc/kernels.hip) at the shapes where its paths
turn over.  The matching kernels assemble the descriptors they stage in LDS from the gradient planes: one scalar pointer per
source row and one byte offset per lane, four columns at a time, with the image-border selects taken only by wavefronts that
hold a border quad.  What they stage is not visible by itself, so the cases compare what is computed from it - the support
candidates (k_support), the dense maps of both sides (k_dense) and the final maps - and the descriptor snapshot of the same
device function (k_expand_all), byte for byte with the CPU oracle.

The pipeline matches every lattice row, from v = candidate_stepsize (5: staged rows 3 and 7) to the last one, and every image
row in the dense stage, so the first and last rows that carry descriptors are staged in every case.

    32 x 32, D = 16         one wavefront holds both image borders: the ballot must take the border path
    35 x 33, 37 x 33        width 3 and 1 mod 4: the last quad straddles W - 3; the plane pitch is no multiple of the width
    80 x 36, D = 24         width a multiple of 16: the pitch has no slack beyond the margins
    515 x 35, D = 64        a second dense tile three columns wide whose right-image segment starts at a clipped, 4-aligned
                            column; two support column blocks, the second nearly empty
    130 x 36, half res.     descriptor rows alternate: the rows without descriptors must still be written (as zeros)
"""
import numpy as np
import pytest

import util
from pyoracle import ElasParams

pytestmark = pytest.mark.gpu

COMPARED = ["desc1", "desc2", "dcan_raw", "wta1", "wta2", "final1", "final2"]

# name -> (seed, W, H, D, subsampling)
CASES = {
    "32x32": (301, 32, 32, 16, 0),
    "35x33": (302, 35, 33, 16, 0),
    "37x33": (303, 37, 33, 16, 0),
    "80x36": (304, 80, 36, 24, 0),
    "515x35": (305, 515, 35, 64, 0),
    "130x36_half": (306, 130, 36, 32, 1),
}

_WANT = {}  # case name -> (pair, support count, oracle stages): the oracle runs once per case


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU; there is no CPU fallback"
    return util.pkg("engine")


def _params(cls, D, sub):
    p = cls.driver(D - 1)
    p.subsampling = sub
    return p


def _want(oracle, name):
    if name not in _WANT:
        seed, W, H, D, sub = CASES[name]
        L, R = util.pkg("synth").make_pair(seed, H, W, D)
        n = oracle.run_stages(_params(ElasParams, D, sub), L, R)
        _WANT[name] = (L, R, n, {k: oracle.stage(k).copy() for k in COMPARED})
    return _WANT[name]


@pytest.mark.parametrize("gpu_filter", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_staged_descriptors_give_the_oracles_stages(eng, oracle, name, gpu_filter):
    """gpu_filter: the lattice filters on the GPU or on the host pool (they sit between the two matching kernels)."""
    seed, W, H, D, sub = CASES[name]
    L, R, n, want = _want(oracle, name)
    assert n >= 3, "the case must get past the support stage: %d support points" % n
    e = eng.StereoEngine(W, H, _params(eng.SvParams, D, sub), keep_debug=True, gpu_filter=True if gpu_filter else None)
    try:
        d1, d2, status = e.process_host(L, R)
        got = {k: e.debug(k) for k in COMPARED}
    finally:
        e.close()
    assert int(status[0]) == n
    bad = []
    for k in COMPARED:
        g, o = got[k], want[k]
        if g.size != o.size or g.dtype.itemsize != o.dtype.itemsize or not np.array_equal(g.view(np.uint8).ravel(), o.view(np.uint8).ravel()):
            bad.append((k, int((g.ravel() != o.ravel()).sum()) if g.size == o.size else -1))
    assert not bad, "stages differ from the oracle: %s" % bad
    assert np.array_equal(d1[0].view(np.uint8).ravel(), want["final1"].view(np.uint8).ravel())
    assert np.array_equal(d2[0].view(np.uint8).ravel(), want["final2"].view(np.uint8).ravel())
    # image rows 0 .. 2 and H-3 .. H-1 carry no descriptors: zeros, in the oracle's images as in the snapshot
    for k in ("desc1", "desc2"):
        rows = got[k].view(np.uint8).reshape(H, W * 16)
        assert want[k].size * want[k].dtype.itemsize == H * W * 16
        assert not rows[:3].any() and not rows[H - 3:].any(), k
        assert rows[3:H - 3].any(), k  # (and the rows between them are not all empty)
