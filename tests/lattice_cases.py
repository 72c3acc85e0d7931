"""Support lattices painted point by point for the GPU lattice filters (csrc/kernels.hip: k_filter_classify, k_filter_resolve,
k_filter_vertical, k_filter_horizontal, k_filter_collect, k_filter_corners), and a plain numpy restatement of what the filters do.

A case is an int16 [Hc][Wc] lattice (row-major, the oracle's and dcan_raw's layout), the image size and lattice step it belongs to, the
filter parameters, and a note of what it is aimed at.  The expected lists come from the oracle (orc_support_filter); the restatement
here exists to PROVE the aims - that a chain really is a chain of uncertain points, that a tie really ties - and is itself compared
with the oracle on every case (test_lattice_filter_edges.py).

Contract of the lattices (sv_gpu_support_filter, sv_debug_inject_lattice): -1 or 0 .. disp_max, lattice row 0 and column 0 all zero.
Those zeros are valid points of disparity 0 for the filters (the collection leaves them out): with incon_window_size 1 and
incon_min_support 3 every point of column 0 and of row 0 is uncertain and hangs on its predecessor, so the border alone is a chain.
The cases below keep their own values at 10 and above where the border must not take part, and say so where it must.

Constants restated from csrc/kernels.hip (the tests read the file and compare): FCL_THREADS = FLT_THREADS = 256 lattice indices per
classify / collect block, strips of 8 lines in the redundancy passes, 16 flag bytes per step of the walk, three refinement rounds."""
import numpy as np

DISP_MAX = 255
BLOCK = 256     # FCL_THREADS, FLT_THREADS
STRIP = 8       # filter_strip()
WALK = 16       # redundancy_walk()
ROUNDS = 3      # k_filter_resolve
NONE, KEEP, DROP, UNC = 0, 1, 2, 3   # FST_*
FAR = 10000000  # elas.cpp:245: the corner search starts from this squared distance


def params(cls, over):
    """The parameters of a case as `cls` (ElasParams or SvParams): what the driver runs, plus the case's overrides."""
    p = cls.driver(DISP_MAX)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def blank(Wc, Hc):
    d = np.full((Hc, Wc), -1, np.int16)
    d[0, :] = 0
    d[:, 0] = 0
    return d


class Case:
    def __init__(self, name, family, lattice, over, aim, step=5, image=None, expect=None):
        self.name, self.family, self.aim, self.step = name, family, aim, step
        self.over = dict(over)
        self.lattice = np.ascontiguousarray(lattice, np.int16)
        self.lattice.setflags(write=False)
        self.Hc, self.Wc = self.lattice.shape
        self.W, self.H = image if image else (self.Wc * step, self.Hc * step)
        assert ((self.W + step - 1) // step, (self.H + step - 1) // step) == (self.Wc, self.Hc), name
        self.expect = dict(expect or {})

    def key(self):
        """Cases of one key may share a launch: one lattice size, one image size, one parameter set."""
        return (self.W, self.H, self.step, tuple(sorted(self.over.items())))

    @property
    def filter_params(self):
        p = dict(incon_window_size=5, incon_threshold=5, incon_min_support=5, add_corners=1)  # the driver's
        p.update({k: v for k, v in self.over.items() if k in p})
        return p["incon_window_size"], p["incon_threshold"], p["incon_min_support"], p["add_corners"]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def classify(lat, win, thr, need):
    """Per point [Hc][Wc]: c_late (consistent neighbours later-or-equal in scan order, u outer / v inner), c_all (in the original
    lattice) and the state: KEEP if c_late >= need, DROP if c_all < need, else UNC; NONE for invalid points."""
    Hc, Wc = lat.shape
    P = np.full((Hc + 2 * win, Wc + 2 * win), -1, np.int32)
    P[win:win + Hc, win:win + Wc] = lat
    d = lat.astype(np.int32)
    c_late, c_all = np.zeros((Hc, Wc), np.int32), np.zeros((Hc, Wc), np.int32)
    for du in range(-win, win + 1):
        for dv in range(-win, win + 1):
            nb = P[win + dv:win + dv + Hc, win + du:win + du + Wc]
            hit = ((nb >= 0) & (np.abs(d - nb) <= thr)).astype(np.int32)
            c_all += hit
            if du > 0 or (du == 0 and dv >= 0):
                c_late += hit
    valid = lat >= 0
    state = np.where(c_late >= need, KEEP, np.where(c_all < need, DROP, UNC))
    return np.where(valid, c_late, 0), np.where(valid, c_all, 0), np.where(valid, state, NONE)


def drop_inconsistent(lat, win, thr, need):
    """elas.cpp:152-176: in place, in scan order.  Points the classification keeps for sure never change and are not visited."""
    _, _, state = classify(lat, win, thr, need)
    D = lat.astype(np.int32).copy()
    Hc, Wc = D.shape
    todo = np.argwhere((state.T == DROP) | (state.T == UNC))  # rows (u, v) in scan order
    for u, v in todo:
        w = D[max(v - win, 0):v + win + 1, max(u - win, 0):u + win + 1]
        if int(((w >= 0) & (np.abs(w - D[v, u]) <= thr)).sum()) < need:
            D[v, u] = -1
    return D


def drop_redundant_vertical(D):
    """elas.cpp:178-233 along the lattice columns (max_dist 5, threshold 1), every column at once, row after row."""
    D = D.copy()
    Hc = D.shape[0]
    for v in range(Hc):
        d = D[v]
        sides = []
        for sgn in (-1, 1):
            s = np.zeros(d.shape, bool)
            for j in range(1, 6):
                v2 = v + sgn * j
                if 0 <= v2 < Hc:
                    s |= (D[v2] >= 0) & (np.abs(d - D[v2]) <= 1)
            sides.append(s)
        D[v] = np.where((d >= 0) & sides[0] & sides[1], -1, d)
    return D


def collect(D, step, W, H, add_corners):
    """elas.cpp:424-428 (u outer, v inner, without lattice row / column 0) and :235-264; returns (list, [(best, ties)] per corner)."""
    uv = np.argwhere(D.T[1:, 1:] >= 0) + 1
    pts = [(int(u) * step, int(v) * step, int(D[v, u])) for u, v in uv]
    corners = []
    if add_corners:
        b = [[0, 0, 0], [0, H - 1, 0], [W - 1, 0, 0], [W - 1, H - 1, 0]]
        for c in b:
            dist = [(c[0] - p[0]) ** 2 + (c[1] - p[1]) ** 2 for p in pts]
            best = min(dist) if dist else FAR
            if best < FAR:
                c[2] = pts[dist.index(best)][2]   # the first of equally near points
            corners.append((best, [j for j, x in enumerate(dist) if x == best and best < FAR]))
        pts = pts + [tuple(c) for c in b] + [(b[2][0] + b[2][2], b[2][1], b[2][2]), (b[3][0] + b[3][2], b[3][1], b[3][2])]
    return np.array(pts, np.int32).reshape(-1, 3), corners


def model(case, parts=False):
    win, thr, need, corners = case.filter_params
    A = drop_inconsistent(case.lattice, win, thr, need)
    B = drop_redundant_vertical(A)
    C = drop_redundant_vertical(B.T).T
    pts, ties = collect(C, case.step, case.W, case.H, corners)
    return (pts, A, B, C, ties) if parts else pts


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
CASES, FAMILIES = {}, {}


def _add(name, family, lattice, over, aim, **kw):
    assert name not in CASES
    CASES[name] = Case(name, family, lattice, over, aim, **kw)
    FAMILIES.setdefault(family, []).append(name)


CHAIN = dict(incon_window_size=1, incon_min_support=3, incon_threshold=1, add_corners=0)
LINKS = 210   # more than 200: three rounds cannot finish them


def _full():
    v, u = np.mgrid[0:60, 0:80]
    d = (2 * ((u + v) % 6)).astype(np.int16)
    d[0, :] = 0
    d[:, 0] = 0
    return d


_add("full_80x60", "full", _full(), {}, "every inner point survives: the list is max_pts long and longer than the bulk copy's head",
     expect=dict(n_main=79 * 59, count=79 * 59 + 6))


def _chain_col(keep):
    d = blank(8, 230)
    d[10:10 + LINKS, 4] = 20
    if keep:
        d[10, 5] = 20
    return d


def _chain_row(keep):
    d = blank(230, 300)
    d[3, 10:10 + LINKS] = 20
    if keep:
        d[4, 10] = 20   # the neighbour (u, v + 1) of the head: later in scan order
    return d


# cells: the chain's own lattice points, [(u, v)]; unc: how many of them the classification leaves uncertain; kept: how many the
# inconsistency pass keeps.  (The extra point of the keeping variants is no chain cell.)
_add("chain_col_drop", "chains", _chain_col(False), CHAIN, "210 equal values down a column: 208 uncertain points at consecutive indices, all dropped one after the other",
     expect=dict(cells=[(4, 10 + i) for i in range(LINKS)], unc=LINKS - 2, kept=0, chain=True))
_add("chain_col_keep", "chains", _chain_col(True), CHAIN, "the same with a neighbour right of the head: 207 uncertain points, each kept because its predecessor was; the last falls",
     expect=dict(cells=[(4, 10 + i) for i in range(LINKS)], unc=LINKS - 3, kept=LINKS - 1, chain=True))
_add("chain_row_drop", "chains", _chain_row(False), CHAIN, "210 equal values along a row: uncertain points Hc = 300 indices apart, classify blocks without any between them",
     expect=dict(cells=[(10 + i, 3) for i in range(LINKS)], unc=LINKS - 2, kept=0, chain=True, sparse_blocks=True))
_add("chain_row_keep", "chains", _chain_row(True), CHAIN, "the same with a neighbour below the head, kept link by link; the last falls",
     expect=dict(cells=[(10 + i, 3) for i in range(LINKS)], unc=LINKS - 2, kept=LINKS - 1, chain=True, sparse_blocks=True))


def _chain_border():
    d = blank(230, 16)
    d[10, 1:1 + LINKS] = 1
    return d


_add("chain_border", "chains", _chain_border(), CHAIN,
     "a row of ones that starts next to column 0: its head is kept by three zeros of the border, the rest link by link; dropped whole if the border did not count",
     expect=dict(cells=[(1 + i, 10) for i in range(LINKS)], unc=LINKS - 1, kept=LINKS - 1, chain=True, border=True))


# classify blocks of 256 indices.  Window 1, three needed: a point with one consistent neighbour before it and one behind it in scan
# order is uncertain.  Each target gets the value 20 and the fewest neighbours (inner points, so far empty) that make it so; a
# target on the border is 0 and gets neighbours of 1, within the threshold.
BLOCKS = dict(incon_window_size=1, incon_min_support=3, incon_threshold=1, add_corners=1)
BLOCK_EDGES = (BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK)


def _blocks(Hc, win, need):
    from itertools import combinations
    Wc = max(4, (3 * BLOCK) // Hc + 3)
    d = blank(Wc, Hc)
    cl = lambda e: classify(e, win, BLOCKS["incon_threshold"], need)[2]
    done = []
    for idx in BLOCK_EDGES:
        u, v = divmod(idx, Hc)
        inner = u >= 1 and v >= 1
        near = range(-win, win + 1)
        cand = [(u + du, v + dv) for du in near for dv in near if (du or dv) and 1 <= u + du < Wc and 1 <= v + dv < Hc and d[v + dv, u + du] < 0]
        for x, combo in ((x, c) for x in ((20, 1) if inner and d[v, u] < 0 else (max(int(d[v, u]), 1),)) for k in range(4) for c in combinations(cand, k)):
            e = d.copy()
            if inner and d[v, u] < 0:
                e[v, u] = x
            for (u2, v2) in combo:
                e[v2, u2] = x
            st = cl(e)
            if st[v, u] == UNC and all(st[q] == UNC for q in done):
                d = e
                break
        else:
            return None
        done.append((v, u))
    return d


for _Hc in (2, 3, 11, 16, 17, 64, 65, 255, 256, 257):
    # (window 1 and three needed wherever that can be done; the last two points of column 0 are never both uncertain within window 1)
    _win, _need, _d = next((w, n, d) for w, n, d in ((w, n, _blocks(_Hc, w, n)) for w, n in ((1, 3), (1, 4), (2, 4), (2, 5), (2, 6))) if d is not None)
    _add("blocks_h%d" % _Hc, "blocks", _d, dict(BLOCKS, incon_window_size=_win, incon_min_support=_need),
         "uncertain points at the last index of a classify block and the first of the next, lattice columns of %d points" % _Hc, expect=dict(unc_at=BLOCK_EDGES))


def _blocks_ends():
    d = blank(16, 64)
    d[2:4, 1] = 30      # a vertical pair: with two needed the lower point hangs on the upper one
    d[10:12, 15] = 40
    return d


_add("blocks_first_last", "blocks", _blocks_ends(), dict(BLOCKS, incon_min_support=2), "four classify blocks, uncertain points in the first and the last only",
     expect=dict(unc_blocks=[0, 3]))


def _edges_lattice():
    rng = np.random.default_rng(41)
    d = np.where(rng.random((20, 24)) < 0.9, rng.integers(0, 4, (20, 24)) * 60, -1).astype(np.int16)
    d[1, 1:] = 60        # row 1, column 1, the last row and the last column are full
    d[1:, 1] = 120
    d[-1, 1:] = 180
    d[1:, -1] = 60
    d[0, :] = 0
    d[:, 0] = 0
    return d


for _win in (0, 1, 5):
    for _need in (0, 1, 60):
        for _thr in (0, 4095):
            _add("edges_w%d_n%d_t%d" % (_win, _need, _thr), "edges", _edges_lattice(), dict(incon_window_size=_win, incon_min_support=_need, incon_threshold=_thr, add_corners=_win % 2),
                 "windows that hang over every edge of the lattice; %s" % ("nothing can be dropped" if _need <= 1 else "sixty needed"), expect=dict(keeps_all=_need <= 1))

# redundancy walks: the inconsistency pass keeps everything (nothing needed), lines of every length at which the walk's 16-flag step
# and the strips of 8 lines turn over
WALKS = dict(incon_min_support=0, add_corners=0)
LINES = (1, 2, 5, 6, 15, 16, 17, 31, 32, 33)
STRIPS = (7, 8, 9, 15, 16, 17)


def _walk_lattice(Wc, Hc, seed):
    rng = np.random.default_rng(seed)
    d = np.where(rng.random((Hc, Wc)) < 0.8, rng.choice([10, 11, 12, 14, 30], (Hc, Wc)), -1).astype(np.int16)
    d[0, :] = 0
    d[:, 0] = 0
    return d


for _i, _n in enumerate(LINES):
    _s = STRIPS[_i % len(STRIPS)]
    _add("walk_v%d_x%d" % (_n, _s), "walks", _walk_lattice(_s, _n, 100 + _n), WALKS, "columns of %d points, %d of them: the vertical pass's walk and its last strip" % (_n, _s))
    _s = STRIPS[(_i + 3) % len(STRIPS)]
    _add("walk_h%d_x%d" % (_n, _s), "walks", _walk_lattice(_n, _s, 200 + _n), WALKS, "rows of %d points, %d of them: the horizontal pass's walk and its last strip" % (_n, _s))


def _runs(transpose):
    """Line L (2..12): a run of L equal values; 13/14: values that alternate by exactly 1 / exactly 2; 15..17: three equal values at
    distances (5, 5), (5, 6), (6, 5)."""
    d = np.full((40, 19), -1, np.int16)
    for L in range(2, 13):
        d[3:3 + L, L] = 20 + 3 * L
    d[3:20, 13] = 100 + (np.arange(17) % 2)
    d[3:20, 14] = 120 + 2 * (np.arange(17) % 2)
    for u, (a, b) in zip((15, 16, 17), ((5, 5), (5, 6), (6, 5))):
        d[[3, 3 + a, 3 + a + b], u] = 200 + 10 * (u - 15)
    if transpose:
        d = np.ascontiguousarray(d.T)
    d[0, :] = 0
    d[:, 0] = 0
    return d


# (neighbouring lines differ by 3 or more, so the pass across the lines drops nothing)
_add("runs_vertical", "walks", _runs(False), WALKS, "runs of 2..12 equal values down the columns, differences of exactly 1 and 2, matches at distance exactly 5 and 6",
     expect=dict(triples=[((15, 3), (5, 5)), ((16, 3), (5, 6)), ((17, 3), (6, 5))], vertical=True))
_add("runs_horizontal", "walks", _runs(True), WALKS, "the same along the rows",
     expect=dict(triples=[((3, 15), (5, 5)), ((3, 16), (5, 6)), ((3, 17), (6, 5))], vertical=False))


def _through():
    d = blank(12, 20)
    for v in (2, 5, 11):      # P at v = 5 has a match above (2); below, X at 8 matches, Q at 11 is too far
        d[v, 4:6] = 50        # ... each with a twin to its right, which the inconsistency pass asks for
    d[8, 4] = 50              # X: alone, dropped by the inconsistency pass
    return d


_add("walk_through_dropped", "walks", _through(), dict(incon_window_size=1, incon_min_support=2, incon_threshold=0, add_corners=0),
     "a point the inconsistency pass drops stood between two that matched only through it: the upper one stays", expect=dict(through=dict(P=(4, 5), X=(4, 8))))

# collection and corner points.  Nothing needed: every painted point survives the inconsistency pass; values 20 apart survive the rest.
COLLECT = dict(incon_min_support=0)
_SURV = [(7, 5, DISP_MAX), (12, 9, 40), (3, 13, 80)]
for _k in (0, 1, 2, 3):
    for _c in (0, 1):
        _d = blank(20, 16)
        for _u, _v, _x in _SURV[:_k]:
            _d[_v, _u] = _x
        _add("collect_%d_c%d" % (_k, _c), "collect", _d, dict(COLLECT, add_corners=_c), "%d points survive%s" % (_k, ", one of them at disp_max" if _k else ""),
             expect=dict(n_main=_k, count=_k + 6 * _c))


def _spread(one_block):
    d = blank(40, 64)   # ten collect blocks
    for n in range(5):
        idx = (BLOCK + 9 + 50 * n) if one_block else ((2 * n + 1) * BLOCK + 37 * n + 70)
        u, v = divmod(idx, 64)
        d[v, u] = 20 + 20 * n
    return d


_add("collect_one_block", "collect", _spread(True), dict(COLLECT, add_corners=1), "five survivors in one collect block of ten", expect=dict(n_main=5, collect_blocks=[1]))
_add("collect_one_per_block", "collect", _spread(False), dict(COLLECT, add_corners=1), "five survivors, one in every other collect block", expect=dict(n_main=5, collect_blocks=[1, 3, 5, 7, 9]))


def _ties():
    """W - 1 and H - 1 are multiples of the step, so that mirrored points are equally far from a corner.  Per corner two points; the
    first in list order carries the LARGER disparity (a key ordered by disparity before position would take the other)."""
    d = blank(20, 16)
    for n, (cu, cv) in enumerate(((0, 0), (0, 15), (19, 0), (19, 15))):
        su, sv = (1 if cu == 0 else -1), (1 if cv == 0 else -1)
        a, b = (cu + su * 1, cv + sv * 2), (cu + su * 2, cv + sv * 1)
        first, second = sorted((a, b))
        d[first[1], first[0]] = 60 + 40 * n
        d[second[1], second[0]] = 40 + 40 * n
    return d


_add("corner_ties", "collect", _ties(), dict(COLLECT, add_corners=1), "two survivors equally far from each image corner: the first in list order gives the corner its disparity",
     image=(96, 76), expect=dict(n_main=8, tied_corners=[0, 1, 2, 3]))


def _far():
    d = blank(213, 3)
    d[1, 1] = 33
    d[2, 3] = 77
    return d


_add("corner_far", "collect", _far(), dict(COLLECT, add_corners=1), "3400 x 48 at step 16: both survivors lie more than sqrt(1e7) pixels from the right-hand corners, which get 0",
     step=16, image=(3400, 48), expect=dict(n_main=2, far_corners=[2, 3]))


# random lattices: the generator of test_capi_and_host.py::test_host_filter_random_lattices within the GPU filters' parameter range
def _random(seed):
    rng = np.random.default_rng(1000 + seed)
    Wc, Hc = int(rng.integers(8, 141)), int(rng.integers(8, 141))
    step = int(rng.choice([3, 5, 6, 8]))
    over = dict(candidate_stepsize=step, incon_window_size=int(rng.integers(0, 6)), incon_threshold=int(rng.integers(1, 8)), incon_min_support=int(rng.integers(1, 13)),
                add_corners=int(rng.integers(0, 2)))
    W, H = Wc * step - int(rng.integers(0, step)), Hc * step - int(rng.integers(0, step))
    noise = rng.integers(0, 60, (Hc, Wc))
    ramp = np.add.outer(np.arange(Hc), np.arange(Wc)) // int(rng.integers(2, 9)) + int(rng.integers(0, 30))
    d = np.where(rng.random((Hc, Wc)) < 0.5, noise, ramp)
    d = np.where(rng.random((Hc, Wc)) < rng.uniform(0.05, 0.9), d, -1).astype(np.int16)
    d[0, :] = 0
    d[:, 0] = 0
    return d, over, step, (W, H)


for _seed in range(24):
    _d, _over, _step, _img = _random(_seed)
    _add("random_%02d" % _seed, "random", _d, _over, "noise / ramp mix, %d x %d" % (_d.shape[1], _d.shape[0]), step=_step, image=_img)

for _c in CASES.values():
    if "candidate_stepsize" not in _c.over:
        _c.over["candidate_stepsize"] = _c.step


# ---- fillers: what shares a launch with a case of its size ----------------------------------------------------------------------------------
def dense_filler(case):
    """Every point valid, values in steps of one: a lattice that leaves thousands of uncertain points, block counts and state words behind."""
    v, u = np.mgrid[0:case.Hc, 0:case.Wc]
    d = ((3 * u + 5 * v) % 7 + (u // 3) % 5).astype(np.int16)
    d[0, :] = 0
    d[:, 0] = 0
    return d


def sparse_filler(case):
    return blank(case.Wc, case.Hc)


def turned_filler(case):
    """The case's own inner lattice turned by 180 degrees."""
    d = case.lattice.copy()
    d[1:, 1:] = case.lattice[1:, 1:][::-1, ::-1]
    return d
