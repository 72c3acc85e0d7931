"""Disparity maps painted pixel by pixel for the second half of the disparity engine - L/R check, speckle removal, gap interpolation,
adaptive mean, median - and the reference chain they are compared with.  The engine takes them through sv_debug_inject (stage "wta": in
front of the L/R check, "lr": in front of speckle removal); the image pair that carries a case is any synth.make_pair of its size that
gets past the support stage.  Pure numpy; nothing is random beyond fixed seeds.

CASES: {name: Case} in a fixed order; FAMILIES: {family: [names]}.  A Case has the two maps (float32 [Hm, Wm], read-only), the stage they
are injected at, the parameter overrides (params(cls, case.over)), the image shape, the "ccl_cap" of sv_debug_set (0: the handle's own)
and `expect`: what the case is aimed at, checked by tests/test_postprocess_edges.py on the injected maps (with the small labelling
of this module) and on the ORACLE's output, so that a case cannot lose its point in silence:

    ("comp", side, (v, u), size, kept)   the component of (v, u) in the injected map has `size` pixels; the oracle's speckle stage keeps / wipes it
    ("run", side, v, u0, u1)             pixels u0 .. u1 of row v are exactly one run of linked pixels
    ("runs", side, band, n)              band `band` (8 rows) of the injected map holds n runs
    ("total_runs", side, n)              the map holds n runs
    ("path", side, (v, u), size)         the component of (v, u) has `size` pixels and is one pixel wide (no pixel has more than two neighbours)
    ("at", stage, side, (v, u), x)       the oracle's map after `stage` holds x at (v, u)
    ("same" | "changed", stage, side, (v, u))   ... holds / does not hold the injected value there
    ("median", (v, u))                   the left map's (v, u) is -10 after the median if the case has one, else what the mean left
    ("differs", stage, stage2)           the oracle's left maps after the two stages differ somewhere
    ("corners", T, line1, line2, line3, g, Ln)   gaps open at the start / the end of the gap lines 1 - 3: filled with add_corners up to g pixels
    ("both",)                            the oracle's speckle stage wipes some valid pixels of the left map and keeps others

chain(oracle, p, stage, m1, m2) applies the oracle's single stages in the order of its pipeline (orc_run_stages) and returns
{"lr1": ..., "final2": ...}; test_postprocess_edges.py pins it to that pipeline byte for byte.

Shapes: widths 64, 65, 127, 129, 130 (W % 64 = 0, 1, 63, 1, 2), heights 33 (four bands of 8 rows and one row), 65 and 67 (column masks cross
row 63 | 64), and 4100 x 33 (65 mask words: the second trip of the 64-word scans).  S = 20 is the speckle size of most cases.

What the contract of sv_debug_inject leaves out: a speckle_sim_threshold of 0.5 cannot be met exactly by integer disparities; its cases have
neighbours that differ by 0 (linked) and by 1 (not linked)."""
import math

import numpy as np

INV = np.float32(-10.0)
DISP_MAX = 31
S = 20
BASE = dict(disp_max=DISP_MAX, lr_threshold=2, speckle_sim_threshold=1.0, speckle_size=S, ipol_gap_width=3, add_corners=0, filter_median=1,
            filter_adaptive_mean=1, postprocess_only_left=0, subsampling=0)
PAIR_SEED, PAIR_D = 11, 24   # synth.make_pair(PAIR_SEED, H, W, PAIR_D): at least six support points at every shape used here
A = (33, 130)
B = (67, 130)
STAGES = ("lr", "speckle", "gap", "amean", "final")


def params(cls, over):
    """The parameters of a case as `cls` (ElasParams or SvParams): the ROBOTICS preset, BASE, the case's overrides."""
    p = cls.preset("robotics")
    for k, v in list(BASE.items()) + list(over.items()):
        setattr(p, k, v)
    return p


def chain(oracle, p, stage, m1, m2):
    """The oracle's stages behind `stage` on the maps m1 / m2 (injected at "wta" or "lr"), as orc_run_stages applies them."""
    sub, both = bool(p.subsampling), not p.postprocess_only_left
    if stage == "wta":
        d1, d2 = oracle.lr_check(p, m1, m2)
    else:
        assert stage == "lr"
        d1, d2 = np.array(m1, np.float32), np.array(m2, np.float32)
    out = {"lr1": d1, "lr2": d2}

    def step(name, fn, on=True):
        nonlocal d1, d2
        if on:
            d1 = fn(d1)
            if both:
                d2 = fn(d2)
        out[name + "1"], out[name + "2"] = d1, d2

    step("speckle", lambda D: oracle.speckle(p, D))
    step("gap", lambda D: oracle.gap(p, D))
    step("amean", lambda D: oracle.adaptive_mean(D, sub), bool(p.filter_adaptive_mean))
    step("final", oracle.median, bool(p.filter_median))
    return out


# ---- a labelling of this module's own: what the layout tests measure the painted maps with ---------------------------------------------
def links(D, thr):
    """(hl, vl): pixel linked to its left / upper neighbour (both valid, |difference| <= thr)."""
    D = D.astype(np.float64)
    ok = D >= 0
    hl, vl = np.zeros(D.shape, bool), np.zeros(D.shape, bool)
    hl[:, 1:] = ok[:, 1:] & ok[:, :-1] & (np.abs(D[:, 1:] - D[:, :-1]) <= thr)
    vl[1:] = ok[1:] & ok[:-1] & (np.abs(D[1:] - D[:-1]) <= thr)
    return hl, vl


def run_starts(D, thr):
    return (D >= 0) & ~links(D, thr)[0]


def components(D, thr):
    """(label [H, W] int, -1 at invalid pixels; {label: size}) by union-find over the pixels, 4-adjacency."""
    H, W = D.shape
    hl, vl = links(D, thr)
    parent = list(range(H * W))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for v, u in zip(*np.nonzero(hl)):
        a, b = find(v * W + u), find(v * W + u - 1)
        parent[max(a, b)] = min(a, b)
    for v, u in zip(*np.nonzero(vl)):
        a, b = find(v * W + u), find((v - 1) * W + u)
        parent[max(a, b)] = min(a, b)
    label = np.full((H, W), -1, np.int64)
    sizes = {}
    for v, u in zip(*np.nonzero(D >= 0)):
        r = find(v * W + u)
        label[v, u] = r
        sizes[r] = sizes.get(r, 0) + 1
    return label, sizes


def neighbours(D, thr):
    """Number of linked 4-neighbours of every pixel."""
    hl, vl = links(D, thr)
    n = hl.astype(int) + vl.astype(int)
    n[:, :-1] += hl[:, 1:]
    n[:-1] += vl[1:]
    return n


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, stage, left, right=None, over=None, ccl_cap=0, expect=()):
        self.name, self.family, self.stage, self.ccl_cap = name, family, stage, ccl_cap
        self.over = dict(over or {})
        self.left = np.ascontiguousarray(left, np.float32)
        self.right = np.ascontiguousarray(self.left[::-1, ::-1] if right is None else right, np.float32)  # (turned by 180 degrees: other bits, other bands)
        assert self.left.shape == self.right.shape
        self.left.setflags(write=False)
        self.right.setflags(write=False)
        self.expect = list(expect)
        self.map_shape = self.left.shape
        sub = self.over.get("subsampling", 0)
        self.image_shape = (2 * self.map_shape[0], 2 * self.map_shape[1]) if sub else self.map_shape

    def handle_key(self):
        """Cases with the same key share a handle: image shape and parameters."""
        return self.image_shape + tuple(sorted(self.over.items()))

    def maps(self, side):
        return self.right if side else self.left


CASES = {}
FAMILIES = {}


def _add(name, family, stage, painted, right=None, **kw):
    left, expect = painted
    assert name not in CASES, name
    CASES[name] = Case(name, family, stage, left, right, expect=expect, **kw)
    FAMILIES.setdefault(family, []).append(name)


def _blank(shape, fill=INV):
    return np.full(shape, fill, np.float32)


class _Paint:
    """A map and the expectations that go with what is painted on it."""

    def __init__(self, shape, fill=INV):
        self.D, self.e = _blank(shape, fill), []

    def run(self, v, u0, u1, val=7, size=None, kept=None, s=S):
        """One run u0 .. u1 (inclusive) of row v; a component by itself unless `size` says what it belongs to."""
        self.D[v, u0:u1 + 1] = val
        self.e.append(("run", 0, v, u0, u1))
        if size is None:
            size = u1 - u0 + 1
        if size:
            self.e.append(("comp", 0, (v, u0), size, size >= s if kept is None else kept))

    def comp(self, v, u, size, s=S):
        self.e.append(("comp", 0, (v, u), size, size >= s))

    def done(self):
        return self.D, self.e


def _turnover(n0=S):
    return (n0 - 1, n0, n0 + 1)


# speckle / size turnover: the three places where the code decides "large"
def _size_one_run(shape=A, s=S):
    p = _Paint(shape)
    for v, n in zip((1, 3, 5), _turnover(s)):
        p.run(v, 3, 3 + n - 1, s=s)
    p.run(32, 100, 100 + s - 1, 9, s=s)  # the last band has one row
    p.run(32, 3, 3 + s - 2, 9, s=s)
    return p.done()


def _size_one_band(shape=A, s=S):
    """Three runs in rows 9 - 11 of band 1 (and 25 - 27 of band 3), stacked: 6 + (n - 12) + 6 pixels."""
    p = _Paint(shape)
    for v0 in (9, 25):
        for i, n in enumerate(_turnover(s)):
            u0 = 3 + 30 * i + (28 if v0 == 25 else 0)  # (band 3: 31, 61, 91 - the second one across a mask-word boundary)
            p.run(v0, u0, u0 + 5, size=n, s=s)
            p.run(v0 + 1, u0, u0 + n - 13, size=0)
            p.run(v0 + 2, u0, u0 + 5, size=0)
    return p.done()


def _size_two_bands(shape=A, s=S):
    """Pieces of a = s / 2 and n - a pixels on either side of a band border: small each, s only together."""
    p = _Paint(shape)
    a = s // 2
    for i, n in enumerate(_turnover(s)):
        u0 = 3 + 30 * i
        p.run(15, u0, u0 + a - 1, size=n, s=s)        # rows 15 | 16
        p.run(16, u0, u0 + n - a - 1, size=0)
        p.run(23, u0 + 1, u0 + n - a, size=n, s=s)    # rows 23 | 24, the upper piece starting one column further right
        p.run(24, u0, u0 + a - 1, size=0)
    return p.done()


def _size_three_bands(shape=A, s=S):
    """A column through rows 14 .. 25 (2 + 8 + 2 pixels in bands 1, 2, 3) and n - 12 more pixels in row 25."""
    p = _Paint(shape)
    for i, n in enumerate(_turnover(s)):
        u0 = 30 + 32 * i  # 30, 62, 94: the second one has its column at bit 62 and its foot across 63 | 64
        p.D[14:26, u0] = 7
        p.D[25, u0:u0 + n - 11] = 7
        p.comp(14, u0, n, s)
        p.comp(25, u0 + n - 12, n, s)
    return p.done()


def _size_tiny():
    """One- and two-pixel components, for speckle_size 1 and 2."""
    def paint(s):
        p = _Paint(A)
        p.run(3, 5, 5, s=s)
        p.run(6, 5, 6, s=s)
        p.D[10:12, 8] = 7
        p.comp(10, 8, 2, s)
        p.D[7:9, 20] = 7  # across the band border
        p.comp(8, 20, 2, s)
        p.run(3, 63, 63, 7, s=s)  # two single pixels on either side of a mask-word boundary: 7 | 9 are not linked
        p.run(3, 64, 64, 9, s=s)
        p.run(32, 129, 129, s=s)
        return p.done()
    return paint


# speckle / mask words
def _words(W):
    p = _Paint((33, W))
    if W > 64 + S:
        p.run(1, 45, 63)         # ends at bit 63
        p.run(3, 64, 83)         # starts at bit 0
        p.run(5, 63, 81)         # starts at bit 63
        p.run(7, 54, 73)         # crosses 63 | 64
        p.run(13, 44, 63)
        p.run(15, 64, 82)
        p.run(11, 40, W - 1)     # a whole word between two partial ones (W = 127: one partial word, up to bit 62)
    if W == 130:
        p.run(9, 111, 129)       # crosses 127 | 128 and ends at W - 1
        p.run(25, 109, 128)      # ... and ends one short of it
    p.run(17, W - (S - 1), W - 1)  # ends at W - 1, W % 64 in {0, 1, 2, 63}
    p.run(19, W - S, W - 1)
    p.run(21, 0, W - 1)
    p.run(23, W - 1, W - 1)
    p.run(23, 0, S - 2)
    p.run(32, 0, S - 2)
    p.run(32, W - S, W - 1)
    return p.done()


def _words_4100():
    """65 mask words: run numbers behind the first 64 words of a row come from the second trip of the prefix scan."""
    W = 4100
    p = _Paint((33, W))
    p.run(1, 4086, 4099, size=20)     # across 4095 | 4096 (words 63 | 64), with the six pixels below
    p.run(2, 4090, 4095, size=0)
    p.D[9, 0:W:2] = 7                 # 2050 single-pixel runs ...
    p.run(10, 4080, 4099, size=30)    # ... the last ten of them joined by the run below, in words 63 and 64
    p.comp(9, 4098, 30)
    p.comp(9, 4078, 1)
    p.comp(9, 0, 1)
    p.e.append(("runs", 0, 1, 2051))
    p.run(17, 4096, 4099, 9, size=20)  # word 64 alone, with sixteen pixels in row 18
    p.run(18, 4084, 4099, 9, size=0)
    p.run(25, 4081, 4099)
    return p.done()


# speckle / vertical links
def _links():
    p = _Paint(A)
    p.run(1, 10, 18, size=19)   # two stacked runs sharing nine columns: one union, the rest suppressed
    p.run(2, 10, 19, size=0)
    p.run(4, 40, 49, size=20)
    p.run(5, 40, 49, size=0)
    # the shared stretch across 63 | 64 with the upper run broken exactly there (7 | 9) and the lower one whole (8): the link at bit 0
    # of word 1 is a new one although bit 63 of word 0 is linked - missed, the seven pixels 64 .. 70 would be a component of their own
    p.run(8, 56, 63, 7, size=30)
    p.run(8, 64, 70, 9, size=30)
    p.run(9, 56, 70, 8, size=0)
    # ... and the other way round
    p.run(12, 56, 70, 8, size=30)
    p.run(13, 56, 63, 7, size=0)
    p.run(13, 64, 70, 9, size=30)
    # the same two across band borders (k_ccl_border), the first at 127 | 128: 8 + 2 + 10 pixels are S only together
    p.run(15, 120, 127, 7, size=20)
    p.run(15, 128, 129, 9, size=20)
    p.run(16, 120, 129, 8, size=0)
    p.run(23, 56, 70, 8, size=30)
    p.run(24, 56, 63, 7, size=0)
    p.run(24, 64, 70, 9, size=30)
    # two runs that both come from the word before and share their first link at bit 0: bit 63 of the lower one (9) is not linked to the 7
    # above it, so the carry into the word is 0 and the link at bit 0 is the one that joins them - inside band 3, and across rows 7 | 8
    p.run(27, 50, 70, 7, size=29)
    p.D[28, 63], p.D[28, 64:71] = 9, 8
    p.e.append(("run", 0, 28, 63, 70))
    p.comp(28, 70, 29)
    p.run(7, 113, 129, 7, size=20)
    p.D[8, 127], p.D[8, 128:130] = 9, 8
    p.e.append(("run", 0, 8, 127, 129))
    p.comp(8, 129, 20)
    # every column shared and linked, across a word boundary and a band border: one union per word
    p.run(31, 50, 59, 7, size=20)
    p.run(32, 50, 59, 7, size=0)
    p.run(31, 100, 129, 7, size=60)
    p.run(32, 100, 129, 7, size=0)
    return p.done()


def _stairs():
    """Staircases one pixel wide: two pixels per row, each row one column further right."""
    p = _Paint(A)
    for v in range(1, 11):
        p.D[v, 5 + v:7 + v] = 7        # 20 pixels
        p.D[v, 58 + v:60 + v] = 7      # 19 pixels, through column 63 | 64
        p.D[v + 16, 120 - v:122 - v] = 7   # 20, descending to the left, through bands 2 and 3
    p.D[10, 69] = INV
    p.comp(1, 6, 20)
    p.comp(10, 15, 20)
    p.comp(1, 59, 19)
    p.comp(10, 68, 19)
    p.comp(17, 119, 20)
    p.comp(26, 110, 20)
    return p.done()


# speckle / topology
def _topo_arms():
    p = _Paint(A)
    # U shapes whose arms join only in the band below (row 8)
    p.D[2:8, 10] = p.D[2:8, 20] = 7
    p.D[8, 10:21] = 7
    p.comp(2, 10, 23)
    p.comp(2, 20, 23)
    p.D[4:8, 30] = p.D[4:8, 40] = 7
    p.D[8, 30:41] = 7
    p.comp(4, 30, 19)
    p.comp(4, 40, 19)
    # ... and only in the band above (row 15)
    p.D[15, 10:21] = 7
    p.D[16:20, 10] = p.D[16:20, 20] = 7
    p.comp(19, 10, 19)
    p.comp(19, 20, 19)
    p.D[15, 40:51] = 7
    p.D[16:21, 40] = p.D[16:21, 50] = 7
    p.comp(20, 40, 21)
    p.comp(20, 50, 21)
    # combs: four teeth of three pixels joined in the band below / above by a spine of 7 / 8 pixels across 63 | 64
    for u0, v_spine, teeth, n in ((58, 8, (5, 8), 19), (78, 8, (5, 8), 20), (58, 23, (24, 27), 19), (78, 23, (24, 27), 20)):
        p.D[v_spine, u0:u0 + n - 12] = 9
        for t in range(4):
            p.D[teeth[0]:teeth[1], u0 + 2 * t] = 9
        p.comp(teeth[0], u0, n)
        p.comp(teeth[0], u0 + 6, n)
    return p.done()


def spiral(shape, val=7.0):
    """A one-pixel-wide rectangular spiral from the top left corner inwards, its arms one pixel apart."""
    H, W = shape
    D = _blank(shape)
    v = u = 0
    D[0, 0] = val
    n, k, idle = 1, 0, 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while idle < 2:
        dv, du = dirs[k % 4]
        moved = 0
        while True:
            v1, u1, v2, u2 = v + dv, u + du, v + 2 * dv, u + 2 * du
            if not (0 <= v1 < H and 0 <= u1 < W) or D[v1, u1] >= 0:
                break
            if 0 <= v2 < H and 0 <= u2 < W and D[v2, u2] >= 0:
                break
            v, u = v1, u1
            D[v, u] = val
            n, moved = n + 1, moved + 1
        idle = idle + 1 if moved == 0 else 0
        k += 1
    return D, n, (v, u)


def _topo_spiral():
    D, n, end = spiral(B)
    return D, [("path", 0, (0, 0), n), ("path", 0, end, n), ("comp", 0, (0, 0), n, True)]


def _topo_touch():
    """Small pieces against a component that is large inside its band."""
    p = _Paint(A)
    p.D[8:16, 10:20] = 7            # 80 pixels in band 1
    p.run(7, 12, 14, size=86)       # three pixels touching it from above, across rows 7 | 8 ...
    p.run(16, 12, 14, size=86)      # ... and from below, across 15 | 16: the two touch only through the large one
    p.comp(8, 10, 86)
    p.run(7, 30, 32)                # and the same pieces next to nothing
    p.run(16, 30, 32)
    p.D[16:24, 60:70] = 9           # a large one across 63 | 64 with small pieces in the same band and in both neighbours
    p.run(15, 62, 65, 9, size=92)
    p.run(24, 62, 65, 9, size=92)
    p.D[20, 70:74] = 9
    p.comp(20, 73, 92)
    p.comp(16, 60, 92)
    return p.done()


# speckle / similarity
def _similar(t):
    """Neighbours differing by floor(t) (linked) and floor(t) + 1 (not linked)."""
    lo, hi = int(math.floor(t)), int(math.floor(t)) + 1
    p = _Paint(A)
    for i, d in enumerate((lo, hi)):
        u0, both = 5 + 49 * i, d <= t  # 5 and 54: the second pair of runs meets at column 63 | 64
        n = 20 if both else 10
        p.D[1, u0:u0 + 10], p.D[1, u0 + 10:u0 + 20] = 7, 7 + d       # horizontally, inside a word and (i = 1) at bit 63 | 64 ...
        p.D[4, u0 - 1:u0 + 9], p.D[4, u0 + 9:u0 + 19] = 7 + d, 7     # ... the larger value first
        p.e += [("run", 0, 1, u0, u0 + n - 1), ("run", 0, 4, u0 - 1, u0 + n - 2)]
        for q in ((1, u0), (1, u0 + 19), (4, u0 - 1), (4, u0 + 18)):
            p.comp(q[0], q[1], n)
        p.run(6, u0, u0 + 9, 7, size=20 if both else 10)            # vertically inside band 0
        p.run(7, u0, u0 + 9, 7 + d, size=0)
        p.run(15, u0, u0 + 9, 7 + d, size=20 if both else 10)       # ... and across a band border
        p.run(16, u0, u0 + 9, 7, size=0)
        p.comp(7, u0, 20 if both else 10)
        p.comp(16, u0, 20 if both else 10)
    # a ramp 0, 1, 2, ... 25 whose ends differ by far more than the threshold, then one in steps of two
    p.D[20, 3:29] = np.arange(26)
    p.comp(20, 3, 26 if t >= 1 else 1)
    p.comp(20, 28, 26 if t >= 1 else 1)
    p.D[22, 3:19] = 2 * np.arange(16)
    p.D[23:27, 18] = 30
    p.comp(22, 3, 20 if t >= 2 else 1)
    p.comp(26, 18, 20 if t >= 2 else 5)
    # pixels linked horizontally but not vertically: two runs of ten, one on the other, their values t + 1 apart
    p.run(29, 40, 49, 5, size=10)
    p.run(30, 40, 49, 5 + hi, size=10)
    return p.done()


# speckle / tables
TABLE_K = 8


def _table(n):
    """Band 0 holds exactly n >= 8 runs, every other band fewer."""
    p = _Paint(A)
    for r in range(8):
        p.run(r, 3 + r, 3 + r + S - 2 + (r & 1), 7 + 3 * (r & 1))   # 19 and 20 pixels in turn, no two linked (7 | 10)
    for i in range(n - 8):
        p.run(0, 60 + 2 * i, 60 + 2 * i)
    p.run(10, 5, 24)
    p.run(18, 5, 23)
    p.run(32, 5, 24)
    p.e.append(("runs", 0, 0, n))
    p.e += [("runs", 0, b, 1) for b in (1, 2, 4)]
    return p.done()


def _table_last_band():
    """Only the last band (row 32) overflows a table of 8; the others hold one run each."""
    p = _Paint(A)
    for b, n in enumerate((20, 19, 20, 19)):
        p.run(8 * b + 1, 5, 5 + n - 1)
    for i in range(9):
        p.run(32, 2 * i, 2 * i)
    p.run(32, 60, 79)
    p.e += [("runs", 0, b, 1) for b in range(4)] + [("runs", 0, 4, 10)]
    return p.done()


def _checker(n):
    """Single pixels in checkerboard order, row by row, and one run of 25 in the last row: n runs in all, at most 521 per band.
    The pool of run records of a 130 x 67 map holds max(130 * 67 / 4, 4096) = 4096."""
    p = _Paint(B)
    v, u = np.nonzero((np.add.outer(np.arange(66), np.arange(130)) & 1) == 0)
    p.D[v[:n - 1], u[:n - 1]] = 7
    p.run(66, 10, 34)
    p.comp(0, 0, 1)
    p.comp(int(v[n - 2]), int(u[n - 2]), 1)
    p.e.append(("total_runs", 0, n))
    return p.done()


def _noise(shape, seed, density):
    rng = np.random.default_rng(seed)
    D = rng.choice(np.array([7, 8, 7, 8, 7, 8, 10, 11], np.float32), shape)  # (three quarters of the valid neighbours are linked)
    D[rng.random(shape) >= density] = INV
    return D, [("both",)]


# gaps: seven lines ten apart, each with its own features; `T`: the lines are columns (the map is painted transposed)
def _gap_lines(shape, g, T, first=2):
    H, W = shape
    M = _blank((W, H) if T else (H, W))
    Ln = M.shape[1]
    e = []
    far = min(65, Ln - 1)  # the end point behind the gap that straddles position 63 | 64

    def seg(line, a, b, val):
        M[line, a:b + 1] = val

    def at(line, pos, val):
        e.append(("at", "gap", 0, (pos, line) if T else (line, pos), np.float32(val)))

    ln = [first + 10 * i for i in range(7)]
    # line 0: gaps of g (filled: 10.5) and g + 1 (not filled) away from everything, and one of g across 63 | 64
    seg(ln[0], 2, 3, 10), seg(ln[0], 4 + g, 5 + g, 11), seg(ln[0], 7 + 2 * g, 8 + 2 * g, 10)
    at(ln[0], 4, 10.5), at(ln[0], 3 + g, 10.5), at(ln[0], 6 + g, INV), at(ln[0], 6 + 2 * g, INV)
    seg(ln[0], far - g - 2, far - g - 1, 10), seg(ln[0], far, Ln - 1 if Ln < 70 else far + 1, 11)
    at(ln[0], far - g, 10.5), at(ln[0], far - 1, 10.5)
    # line 1: open at the start by g pixels; a gap of g + 1 across 63 | 64
    seg(ln[1], g, g + 1, 12)
    seg(ln[1], far - g - 3, far - g - 2, 10), seg(ln[1], far, Ln - 1 if Ln < 70 else far + 1, 11)
    at(ln[1], far - g - 1, INV), at(ln[1], far - 1, INV)
    # line 2: open at the start by g + 1, at the end by g
    seg(ln[2], g + 1, g + 2, 12), seg(ln[2], Ln - 2 - g, Ln - 1 - g, 14)
    # line 3: open at the end by g + 1; valid at position 0
    seg(ln[3], 0, 0, 12), seg(ln[3], Ln - 3 - g, Ln - 2 - g, 14)
    e.append(("corners", T, ln[1], ln[2], ln[3], g, Ln))
    # line 4: one valid pixel
    seg(ln[4], 30, 30, 9)
    # lines 5 and 6: end values 2, 3 and 4 apart around gaps of two pixels, the larger value behind / in front
    for i, d in enumerate((2, 3, 4)):
        a = 2 + 14 * i
        want = 10 + d / 2 if d < 3 else 10
        seg(ln[5], a, a + 1, 10), seg(ln[5], a + 4, a + 5, 10 + d)
        seg(ln[6], a, a + 1, 10 + d), seg(ln[6], a + 4, a + 5, 10)
        at(ln[5], a + 2, want), at(ln[5], a + 3, want), at(ln[6], a + 2, want), at(ln[6], a + 3, want)
    return (np.ascontiguousarray(M.T) if T else M), e


def _gap_interplay():
    """g = 3.  A pixel that rows and columns could both fill (rows come first), and a row-filled pixel that becomes a column's end point."""
    D = _blank((33, 65))
    D[10, 20:22], D[10, 23:25] = 10, 14          # (10, 22): the row gives min(10, 14) = 10 ...
    D[9, 22] = D[11, 22] = 20                    # ... the column would give 20
    D[20, 40:43], D[20, 45:48] = 10, 10          # (20, 43) and (20, 44) are filled with 10 by the row ...
    D[24, 43] = 12                               # ... and (21 .. 23, 43) by the column between that 10 and this 12: 11
    D[20, 60:63] = 10                            # (20, 63) | (20, 64): the last word has one pixel
    D[20, 64] = 11
    e = [("at", "gap", 0, (10, 22), np.float32(10)), ("at", "gap", 0, (20, 43), np.float32(10)), ("at", "gap", 0, (22, 43), np.float32(11)),
         ("at", "gap", 0, (23, 44), INV), ("at", "gap", 0, (20, 63), np.float32(10.5))]
    return D, e


def _gap_4100(corners):
    """g = 5000: one valid pixel near each end of a row and 63 empty words between them; a row with one valid pixel."""
    D = _blank((33, 4100))
    D[5, 3], D[5, 4096] = 10, 11
    D[20, 4099] = 12
    e = [("at", "gap", 0, (5, 4), np.float32(10.5)), ("at", "gap", 0, (5, 2048), np.float32(10.5)), ("at", "gap", 0, (5, 4095), np.float32(10.5)),
         ("at", "gap", 0, (12, 2048), np.float32(11.25) if corners else INV)]  # (corners: between two row-filled pixels, 10.5 and 12)
    e += [("at", "gap", 0, q, np.float32(x) if corners else INV) for q, x in (((5, 0), 10), ((5, 4099), 11), ((20, 4098), 12), ((20, 0), 12))]
    return D, e


# L/R check
def _lr(shape, sub, thr, seed):
    """Rows 0 .. 15: one scenario per row and side (side 0 in even rows); rows 17 and below: seeded values of every kind."""
    H, W = shape
    M = [_blank(shape), _blank(shape)]
    e = []

    def partner(side, u, d):
        x = (u + d / 2.0 if side else u - d / 2.0) if sub else float(u + d if side else u - d)
        return int(x) if 0 <= x < W else None

    def put(v, side, u, d, dp, want):
        M[side][v, u] = d
        i = partner(side, u, d)
        if i is None:
            assert dp is None
        else:
            for j in (i - 1, i + 1):   # a neighbouring column read by mistake (d / 2 rounded, a column off by one) gives another verdict
                if 0 <= j < W:
                    M[1 - side][v, j] = 25 if want >= 0 else d
            M[1 - side][v, i] = dp
        e.append(("at", "lr", side, (v, u), np.float32(want)))

    for side in (0, 1):
        r = side
        if sub:  # the map is half size, the disparities are full-resolution pixels: u -+ d / 2, truncated towards zero after the range test
            edge_in, edge_out = ((W - 3, 5), (W - 2, 4)) if side else ((3, 5), (2, 5))  # W - 0.5 | W and 0.5 | -0.5
            d0 = 7
        else:
            edge_in, edge_out = ((W - 6, 5), (W - 5, 5)) if side else ((5, 5), (4, 5))  # u + d = W - 1 | W and u - d = 0 | -1
            d0 = 6
        put(r, side, edge_in[0], edge_in[1], edge_in[1], edge_in[1])
        put(r + 2, side, edge_out[0], edge_out[1], None, -10)
        put(r + 4, side, 20, d0, d0 + thr, d0)          # partners exactly lr_threshold apart ...
        put(r + 6, side, 20, d0, d0 + thr + 1, -10)     # ... and one more
        put(r + 8, side, 20, d0, d0 - thr, d0)
        put(r + 10, side, 20, d0, d0 - thr - 1, -10)
        put(r + 12, side, 20, d0, -10, -10)             # invalid partners: no triangle, no match
        put(r + 14, side, 20, d0, -1, -10)
    rng = np.random.default_rng(seed)
    kinds = np.array([-10, -1] + list(range(0, 13)), np.float32)
    for side in (0, 1):
        M[side][17:] = rng.choice(kinds, (H - 17, W))
    return M[0], M[1], e


# mean and median: the workgroup tiles of k_amean are 64 x 32 (tasks of 8 centres), those of k_amean_sub and k_median 64 x 32 (k_median:
# column and row pairs); the filters leave a frame of 3 / 4 pixels alone
def _edges(shape):
    H, W = shape
    return [v for v in (3, 4, 31, 32, 63, 64, H - 5, H - 4) if v < H], [u for u in (3, 4, 63, 64, 127, 128, W - 5, W - 4) if u < W]


def _filt_islands(shape):
    """Isolated valid pixels among invalid ones at the tile edges: the mean leaves them, the median makes them -10."""
    D = _blank(shape)
    vs, us = _edges(shape)
    pts = [(v, u) for i, v in enumerate(vs) for j, u in enumerate(us) if (i + j) % 2 == 0]
    for v, u in pts:
        D[v, u] = 9
    inner = [(v, u) for v, u in pts if 4 <= v < shape[0] - 4 and 4 <= u < shape[1] - 4]
    return D, [("at", "amean", 0, q, np.float32(9)) for q in inner[:4]] + [("median", q) for q in inner[:4]]


def _filt_holes(shape):
    """Isolated holes in a slowly varying valid map at the tile edges: an invalid pixel stays invalid through both filters."""
    H, W = shape
    D = (8 + (np.add.outer(np.arange(H), np.arange(W)) // 5) % 4).astype(np.float32)
    vs, us = _edges(shape)
    pts = [(v, u) for i, v in enumerate(vs) for j, u in enumerate(us) if (i + j) % 2 == 1]
    for v, u in pts:
        D[v, u] = INV
    return D, [("at", "final", 0, q, INV) for q in pts[:6]] + [("at", "amean", 0, q, INV) for q in pts[:6]]


STEPS = (1, 2, 7, 8)  # the mean's weight is 4 up to a difference of 1, 2 from 2 to 7 and 0 from 8 (elas.cpp:1329 keeps five exponent bits)


def _filt_steps(shape):
    """Steps of 1, 2, 7 and 8 along the tile edges x = 63 | 64 and 127 | 128 (one step height per block of rows) and y = 31 | 32 and
    63 | 64 (one per block of columns).  Across a step of 8 the weight is 0: the mean leaves both sides of it as they are."""
    H, W = shape
    v, u = np.mgrid[0:H, 0:W]
    sv = np.array(STEPS)[(v >= 12).astype(int) + (v >= 24) + (v >= 48)]    # blocks whose borders stay eight pixels clear of the tile edges
    su = np.array(STEPS)[(u >= 40).astype(int) + (u >= 90) + (u >= 110)]
    D = (12 + sv * ((u >= 64) & (u < 128)) + su * ((v >= 32) & (v < 64))).astype(np.float32)
    # rows 55 and 42 lie in the blocks with steps of 8 and of 7, eight rows of one value above and below them
    e = [("same", "amean", 0, (55, 63)), ("same", "amean", 0, (55, 64)), ("changed", "amean", 0, (42, 63)), ("changed", "amean", 0, (42, 64))] if H > 60 else []
    return D, e


def _plus_one(D):
    return np.where(D >= 0, D + 1, INV).astype(np.float32)


def _build():
    sp = "speckle"
    # speckle removal
    _add("size_one_run", "size", "lr", _size_one_run())
    _add("size_one_band", "size", "lr", _size_one_band())
    _add("size_two_bands", "size", "lr", _size_two_bands())
    _add("size_three_bands", "size", "lr", _size_three_bands())
    _add("size_s1", "size", "lr", _size_tiny()(1), over=dict(speckle_size=1))
    _add("size_s2", "size", "lr", _size_tiny()(2), over=dict(speckle_size=2))
    for W in (130, 64, 65, 127):
        _add("words_%d" % W, "words", "lr", _words(W))
    _add("words_4100", "words", "lr", _words_4100())
    _add("links_stacked", "links", "lr", _links())
    _add("links_stairs", "links", "lr", _stairs())
    _add("topo_arms", "topology", "lr", _topo_arms())
    _add("topo_spiral", "topology", "lr", _topo_spiral())
    _add("topo_touch", "topology", "lr", _topo_touch())
    for t in (0.5, 1.0, 2.0):
        _add("similar_%g" % t, "similarity", "lr", _similar(t), over=dict(speckle_sim_threshold=t) if t != 1.0 else None)
    for name, painted in (("table_k", _table(TABLE_K)), ("table_k_plus_1", _table(TABLE_K + 1)), ("table_last_band", _table_last_band())):
        _add(name, "tables", "lr", painted, right=_plus_one(painted[0]), ccl_cap=TABLE_K)
    for n in (4096, 4097):
        painted = _checker(n)
        _add("table_pool_%d" % n, "tables", "lr", painted, right=_plus_one(painted[0]))
    _add("noise_129", sp + "_noise", "lr", _noise((33, 129), 1, 0.6))
    _add("noise_65x64", sp + "_noise", "lr", _noise((65, 64), 2, 0.5))
    _add("noise_65x64_cap", sp + "_noise", "lr", _noise((65, 64), 3, 0.7), ccl_cap=64)
    _add("sides_different", "sides", "lr", _size_one_band(), right=_links()[0])
    _add("sides_only_left", "sides", "lr", (_size_two_bands()[0], _size_two_bands()[1] + [("at", "final", 1, (1, 10), np.float32(7))]),
         right=_links()[0], over=dict(postprocess_only_left=1))
    s_half = int(math.sqrt(float(S)) * 2)  # elas.cpp:1017-1022: 8
    half = _Paint(A)
    for painted in (_size_one_run(A, s_half), _size_two_bands(A, s_half)):
        half.D[painted[0] >= 0] = 7
        half.e += painted[1]
    _add("sides_half", "sides", "lr", half.done(), over=dict(subsampling=1))
    # gap interpolation: speckle_size 0, so that the painted map reaches the stage as it is
    for g in (3, 7):
        for c in (0, 1):
            over = dict(speckle_size=0, ipol_gap_width=g, add_corners=c)
            _add("gap_rows_g%d_c%d" % (g, c), "gaps", "lr", _gap_lines(B, g, False), over=over)
            _add("gap_cols_g%d_c%d" % (g, c), "gaps", "lr", _gap_lines(B, g, True, first=62), over=over)
    _add("gap_cols_h65_g3_c1", "gaps", "lr", _gap_lines((65, 64), 3, True), over=dict(speckle_size=0, ipol_gap_width=3, add_corners=1))
    _add("gap_cols_h65_g7_c0", "gaps", "lr", _gap_lines((65, 64), 7, True), over=dict(speckle_size=0, ipol_gap_width=7, add_corners=0))
    _add("gap_interplay", "gaps", "lr", _gap_interplay(), over=dict(speckle_size=0))
    _add("gap_4100", "gaps", "lr", _gap_4100(0), over=dict(speckle_size=0, ipol_gap_width=5000))
    _add("gap_4100_corners", "gaps", "lr", _gap_4100(1), over=dict(speckle_size=0, ipol_gap_width=5000, add_corners=1))
    # L/R check: k_lr (odd width), k_lr2<false> (even), k_lr2<true> (half resolution)
    for name, shape, sub, thr in (("lr_odd_65", (33, 65), 0, 2), ("lr_even_64", (33, 64), 0, 2), ("lr_even_130_t1", A, 0, 1), ("lr_half_130", A, 1, 2),
                                  ("lr_half_65", (33, 65), 1, 2)):
        m1, m2, e = _lr(shape, sub, thr, len(CASES))
        over = dict(lr_threshold=thr, subsampling=sub)
        _add(name, "lr", "wta", (m1, e), right=m2, over={k: v for k, v in over.items() if v != BASE[k]})
    # adaptive mean and median: speckle_size 0 and gap width 0, each filter off in turn, and the half-resolution kernels
    still = dict(speckle_size=0, ipol_gap_width=0)
    for tag, over in (("", {}), ("_mean_only", dict(filter_median=0)), ("_median_only", dict(filter_adaptive_mean=0)), ("_half", dict(subsampling=1))):
        for what, painter in (("islands", _filt_islands), ("holes", _filt_holes), ("steps", _filt_steps)):
            shape = A if tag == "_half" else B
            D, e = painter(shape)
            if tag == "_half":  # gap width 0 becomes 0 / 2 + 1 = 1 at half resolution: single holes would be filled, and other weights
                e = [x for x in e if x[0] == "median"] or [("differs", "final", "gap")]
            _add("filt_%s%s" % (what, tag), "filters", "lr", (D, e), over=dict(still, **over))


_build()


def names(family=None):
    return [n for n in CASES if family is None or CASES[n].family == family]
