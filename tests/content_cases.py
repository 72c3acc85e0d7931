"""Seeded image pairs whose CONTENT is what the disparity engine's other tests never vary: exact ties between disparities, descriptor
bytes at 0 and 255, matches at the very ends of the disparity range, pairs without a consistent match, maps that are half empty.
Pure numpy (plus the package's own synth.make_pair for the textured halves of the mixed pairs); nothing here is random beyond the fixed seeds.

keys() lists the cases, spec(key) is a case without its images, make(key) builds one (cached): (key, preset, parameter overrides, L, R);
cases() yields them all;
params(cls, preset, overrides) makes the ElasParams / SvParams of a case; digest_key(key) is the case's entry in ref_digests.json.
Every pair is between 72 x 160 and 100 x 260 (the compiled reference needs more than 40 rows), disp_max between 15 and 63.

The families (FAMILY[key]) and what each is for - tests/test_content_edges.py asserts it on the oracle's stages, and its
docstrings record what it measured:

rowconst    L[v, u] = f(v), R = L.  The vertical gradients pass the texture gates, and every disparity has the same energy at every
            pixel: only the order of the search decides.
periodic    a random tile of period p along u, R = L shifted by d0: d0, d0 + p, d0 + 2p ... tie exactly.  The ranges hold one to
            four of them; d0 + p exactly at disp_max, and at disp_max + 1.
binary      random 0 / 255 blocks of 1, 2 and 4 pixels and a checkerboard (R shifted by 7 / 3): Sobel responses clip at both ends.
constant    128 and 255 everywhere.
edge        blurred noise; R = L (disparity 0), R shifted by exactly disp_max, by disp_max + 1, and a true disparity of 5 with
            disp_min = 6.
unrelated   independent textures left and right, disp_max 63 (with 31 the driver preset's priors keep more than half of the matches
            consistent on every seed tried; seed "a" does so with 63 as well): the left/right check removes most of what was matched, speckle removal and gap
            interpolation work on the crumbs.  (ROBOTICS gets support_threshold 1 and incon_min_support 1: with its own values it
            finds two support points on this pair, fewer than three, and nothing after the support stage would run; and speckle_size 30: with
            200 no segment survives and gap interpolation has nothing to do.)
mixed       one half synth.make_pair texture, the other constant / row-constant / periodic, across a vertical and a horizontal seam:
            support on one side only, long triangles across the other.  (ROBOTICS with add_corners = 1 - without the corner points
            no triangle can leave the textured side.)
texture     lattice step 10.  Rows 10 j - 3 .. 10 j + 3 are constant along u and form a ramp whose descriptor at the lattice points
            of row 10 j sums to exactly 9 (j = 1 .. 3), 10 (j = 4 .. 6) and 11 (j = 7 .. 9) against support_texture = 10; the three
            rows between hold noise, which only the four corner blocks of the matching window see: the gate alone decides.  (A pure
            ramp cannot do this: all its disparities tie, and a tie never becomes a support point.)
noise       noise_cases() of tests/test_oracle_vs_ref.py."""
import zlib

import numpy as np

import util

SHAPE = (84, 202)        # most cases: a width that is no multiple of 4
SHAPE_PERIODIC = (76, 180)
SHAPE_TEXTURE = (100, 220)
SEAM_U, SEAM_V = 100, 40  # the mixed pairs' seams (lattice column 20, lattice row 8)


def _seed(name):
    return zlib.crc32(name.encode())


def _rng(name):
    return np.random.default_rng(_seed(name))


def _blur(a):
    """(4 x centre + 4 neighbours) / 8 of an array with a one-pixel margin."""
    a = a.astype(np.float64)
    b = (a[:-2, 1:-1] + a[2:, 1:-1] + a[1:-1, :-2] + a[1:-1, 2:] + 4 * a[1:-1, 1:-1]) / 8.0
    return np.clip(np.rint(b), 0, 255).astype(np.uint8)


def _texture(name, H, W):
    return _blur(_rng(name).integers(0, 256, (H + 2, W + 2)))


def _shifted(tex, W, d):
    """(L, R) of a texture at least W + d wide: R(u) = L(u + d), so a left pixel u matches the right pixel u - d."""
    return np.ascontiguousarray(tex[:, :W]), np.ascontiguousarray(tex[:, d:d + W])


def _rowconst(name, H, W):
    f = _rng(name).integers(0, 256, H).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(f[:, None], (H, W)))


def _periodic_tex(name, H, W, p):
    tile = _rng(name).integers(0, 256, (H, p)).astype(np.uint8)
    return np.tile(tile, (1, -(-W // p)))[:, :W]


def _blocks(name, H, W, b):
    cells = _rng(name).integers(0, 2, (-(-H // b), -(-W // b))).astype(np.uint8) * 255
    return np.repeat(np.repeat(cells, b, axis=0), b, axis=1)[:H, :W]


def _checker(H, W, b):
    v, u = np.mgrid[0:H, 0:W]
    return ((((v // b) + (u // b)) & 1) * 255).astype(np.uint8)


def _texture_ramp(name, H, W, d0):
    """See the module docstring, family "texture"."""
    rng = _rng(name)
    tex = np.zeros((H, W + d0), np.uint8)
    for r in range(H):
        j, k = (r + 3) // 10, (r + 3) % 10  # k = 0 .. 6: rows 10 j - 3 .. 10 j + 3
        if k > 6:
            tex[r] = rng.integers(0, 256, W + d0)
            continue
        a4 = 3 if j <= 3 else (4 if j <= 6 else 5)
        tex[r] = 20 * j + [0, 0, 0, 2, 3, a4, a4][k]
    return _shifted(tex, W, d0)


def _mixed(name, other, seam):
    """Left / upper half from synth.make_pair (disparities 2 .. 24), right / lower half `other` in both images."""
    H, W = SHAPE
    L, R = util.pkg("synth").make_pair(_seed(name) % 100000, H, W, 32)
    if other == "constant":
        oL = oR = np.full((H, W), 90, np.uint8)
    elif other == "rowconst":
        oL = oR = _rowconst(name, H, W)
    else:  # period 4, shift 2: at least two exact candidates wherever the support search runs at all (it needs ten disparities)
        oL, oR = _shifted(_periodic_tex(name, H, W + 2, 4), W, 2)
    L, R = L.copy(), R.copy()
    if seam == "v":
        L[:, SEAM_U:], R[:, SEAM_U:] = oL[:, SEAM_U:], oR[:, SEAM_U:]
    else:
        L[SEAM_V:], R[SEAM_V:] = oL[SEAM_V:], oR[SEAM_V:]
    return L, R


def spec(key):
    """(family, preset, overrides, (H, W)) of the case `key` = family_variant_preset, without building its images."""
    fam, *var, preset = key.split("_")
    var = "_".join(var)
    over, shape = {"disp_max": 31}, SHAPE
    if fam == "periodic":
        over, shape = {"disp_max": int(var.split("-")[2][1:])}, SHAPE_PERIODIC
    elif fam == "edge" and var == "belowmin":
        over["disp_min"] = 6
    elif fam == "unrelated":
        over["disp_max"] = 63
        if preset == "robotics":
            over.update(support_threshold=1.0, incon_min_support=1, speckle_size=30)
    elif fam == "mixed" and preset == "robotics":
        over["add_corners"] = 1
    elif fam == "texture":
        over["candidate_stepsize"] = 10
        shape = SHAPE_TEXTURE
    elif fam == "noise":
        shape = (100, 260)
    return fam, preset, over, shape


def _build(key):
    """(L, R) of the case `key`; the images of a case do not depend on its preset."""
    fam, *var, _ = key.split("_")
    var = "_".join(var)
    name = fam + "_" + var
    H, W = spec(key)[3]
    if fam == "rowconst":
        L = R = _rowconst(name, H, W)
    elif fam == "periodic":
        p, d0, _ = [int(x[1:]) for x in var.split("-")]
        L, R = _shifted(_periodic_tex(name, H, W + d0, p), W, d0)
    elif fam == "binary":
        if var == "checker4":
            L, R = _shifted(_checker(H, W + 3, 4), W, 3)
        else:
            L, R = _shifted(_blocks(name, H, W + 7, int(var[5:])), W, 7)
    elif fam == "constant":
        L = R = np.full((H, W), int(var), np.uint8)
    elif fam == "edge":
        d = EDGE_SHIFT[var]
        L, R = _shifted(_texture(name, H, W + d), W, d)
    elif fam == "unrelated":
        L, R = _texture(name + "_left", H, W), _texture(name + "_right", H, W)
    elif fam == "mixed":
        seam, other = var.split("-")
        L, R = _mixed(name, other, seam)
    elif fam == "texture":
        L, R = _texture_ramp(name, H, W, 4)
    elif fam == "noise":
        import test_oracle_vs_ref
        _, _, L, R = {c[0]: c for c in test_oracle_vs_ref.noise_cases()}[key]
    else:
        raise KeyError(key)
    assert L.shape == R.shape == (H, W) and L.dtype == R.dtype == np.uint8, key
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


EDGE_SHIFT = {"zero": 0, "atmax": 31, "pastmax": 32, "belowmin": 5}  # the true disparity of the "edge" pairs (disp_max 31)

_PERIODIC = ["p16-d3-m15",   # one candidate: 3
             "p16-d3-m19",   # two: 3 and 19 = disp_max exactly
             "p16-d3-m18",   # 19 = disp_max + 1: one again
             "p8-d5-m23",    # three: 5, 13, 21
             "p4-d2-m15",    # four: 2, 6, 10, 14
             "p24-d5-m28"]   # 29 = disp_max + 1

_KEYS = (["rowconst_a_driver", "rowconst_a_robotics"]
         + ["periodic_%s_driver" % v for v in _PERIODIC] + ["periodic_p16-d3-m19_robotics", "periodic_p8-d5-m23_robotics"]
         + ["binary_block1_driver", "binary_block1_robotics", "binary_block2_driver", "binary_block4_robotics", "binary_checker4_driver", "binary_checker4_robotics"]
         + ["constant_%d_%s" % (c, pr) for c in (128, 255) for pr in ("driver", "robotics")]
         + ["edge_%s_%s" % (v, pr) for v in ("zero", "atmax", "pastmax", "belowmin") for pr in ("driver", "robotics")]
         + ["unrelated_b_driver", "unrelated_b_robotics"]
         + ["mixed_v-constant_driver", "mixed_v-rowconst_robotics", "mixed_v-periodic_driver", "mixed_h-constant_robotics", "mixed_h-rowconst_driver", "mixed_h-periodic_robotics"]
         + ["texture_ramp_driver", "texture_ramp_robotics"]
         + ["noise_robotics", "noise_middlebury"])

FAMILY = {k: k.split("_")[0] for k in _KEYS}
_CACHE = {}


def keys(family=None):
    return [k for k in _KEYS if family is None or FAMILY[k] == family]


def make(key):
    """(key, preset, overrides, L, R); the arrays are shared between callers: do not write to them."""
    if key not in _CACHE:
        _, preset, over, _ = spec(key)
        L, R = _build(key)
        L.setflags(write=False)
        R.setflags(write=False)
        _CACHE[key] = (key, preset, over, L, R)
    return _CACHE[key]


def cases():
    for k in _KEYS:
        yield make(k)


def params(cls, preset, over):
    """The parameters of a case as `cls` (ElasParams or SvParams)."""
    p = cls.driver(over["disp_max"]) if preset == "driver" else cls.preset(preset)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def digest_key(key):
    return "content_" + key
