"""Deterministic corpus of structured vertex sets and image pairs for the triangulation and everything behind it: the
degeneracies random draws almost never produce.  No randomness except fixed-seed shuffles (the seed is a CRC of the set's name).

sets() yields (name, xy int32 (n, 2)).  Every family comes in sorted and in shuffled order; the families a right image can produce
(x = u - d) also come translated to negative x.  The sanitizer / emulation programs read the same sets from a file
(tests/corpus_file.h).  Coordinates stay inside what sv_create admits (x from -1023 to 8191, y to 4095); the lines of 4000 points use a
step below the lattice's 5 for that.

pair_cases() / make_pair() give small synthetic image pairs whose SUPPORT SET is degenerate (ROBOTICS preset, add_corners = 0): one
textured band on one lattice row or column of an otherwise flat image (no triangle on both sides / on the left side only), a complete
support lattice, and a strip of two lattice rows at the smallest admitted height."""
import zlib

import numpy as np

STEP = 5
X_MIN, X_MAX, Y_MAX = -1023, 8191, 4095   # the coordinate box sv_create admits (W <= 8192, disp_max <= 1023, H <= 4096)
DG_SUB_MAX = 4000                          # csrc/delaunay_gpu.hip: vertices one workgroup triangulates in LDS
DG_PREP_MAX = 4096                         # ... and prepares (dg_prepare)
CUT_SUB_MAX = 50                           # SV_DG_SUBMAX of the cut-path tests; CUT_LATTICES reach cut depths 1 .. 6 with it
CUT_LATTICES = [(10, 10), (20, 10), (20, 20), (40, 20), (40, 40), (64, 50)]
KITTI_GRID = (248, 75)                     # complete support lattice of a 1242 x 375 image, step 5
GRID_4K = (768, 432)                       # ... of a 3840 x 2160 image


def cut_depth(m, sub_max):
    """delaunay_gpu.hip: dg_cut_depth."""
    c = 0
    while ((m + (1 << c) - 1) >> c) > sub_max:
        c += 1
    return c


def _arr(pts):
    return np.asarray(pts, dtype=np.int64).reshape(-1, 2)


def _lattice(w, h, x0=0, y0=0, step=STEP):
    """Complete w x h lattice in the scan order of the support list (u outer, v inner: elas.cpp:422-433)."""
    u, v = np.meshgrid(np.arange(w), np.arange(h), indexing="ij")
    return np.stack([x0 + u.ravel() * step, y0 + v.ravel() * step], 1)


def _line(n, kind):
    k = np.arange(n)
    if kind == "row":
        s = STEP if n * STEP <= 8000 else 2
        return np.stack([k * s, np.full(n, 35)], 1)
    if kind == "col":
        s = STEP if n * STEP <= Y_MAX else 1
        return np.stack([np.full(n, 40), k * s], 1)
    if kind == "diag":
        s = STEP if n * STEP <= Y_MAX else 1
        return np.stack([k * s, k * s], 1)
    if kind == "slope":  # (5k, 10k): neither an axis nor the main diagonal
        return np.stack([k * STEP, k * 2 * STEP], 1) if n * 2 * STEP <= Y_MAX else np.stack([k * 2, k], 1)
    raise ValueError(kind)


def _families():
    """(name, points, may appear in a right image) in sorted (generation) order."""
    # ---- collinear, with and without coincident points
    for kind in ("row", "col", "diag", "slope"):
        for n in (3, 4, 64, 65, 300, 4000):
            p = _line(n, kind)
            yield "collinear_%s_%d" % (kind, n), p, kind == "row"
            if n in (3, 4, 65, 300):
                dup = np.concatenate([p, p[:: max(1, n // 7)], p[:1], p[-1:]])  # every 7th point twice, the ends three times
                yield "collinear_%s_%d_coincident" % (kind, n), dup, kind == "row"
    # ---- the smallest sets
    yield "small_triangle", _arr([[0, 0], [10, 0], [5, 15]]), True
    yield "small_triangle_cw", _arr([[0, 0], [5, 15], [10, 0]]), True
    yield "small_unit_square", _arr([[0, 0], [5, 0], [0, 5], [5, 5]]), True
    for k, extra in enumerate([[5, 5], [0, 5], [10, 5], [20, 5]]):
        yield "small_three_collinear_plus_one_%d" % k, _arr([[0, 0], [5, 0], [10, 0]] + [extra]), True
    yield "small_three_collinear_col_plus_one", _arr([[10, 0], [10, 5], [10, 10], [15, 5]]), True
    # ---- fans: a long collinear run and one point off the line, on either side and at either end
    for n in (7, 64, 300):
        row, col = _line(n, "row"), _line(n, "col")
        for where, q in (("above_first", [0, 30]), ("below_first", [0, 40]), ("above_last", [(n - 1) * STEP, 30]), ("below_last", [(n - 1) * STEP, 40]),
                         ("above_mid", [(n // 2) * STEP, 0]), ("below_mid", [(n // 2) * STEP, 400])):
            yield "fan_row_%d_%s" % (n, where), np.concatenate([row, _arr([q])]), True
        for where, q in (("left_first", [35, 0]), ("right_first", [45, 0]), ("left_last", [35, (n - 1) * STEP]), ("right_last", [45, (n - 1) * STEP]),
                         ("left_mid", [0, (n // 2) * STEP]), ("right_mid", [900, (n // 2) * STEP])):
            yield "fan_col_%d_%s" % (n, where), np.concatenate([col, _arr([q])]), False
    # ---- strips: two and three complete lattice rows / columns
    for rows in (2, 3):
        for n in (2, 3, 50, 301):
            yield "strip_%d_rows_%d" % (rows, n), _lattice(n, rows), True
            yield "strip_%d_cols_%d" % (rows, n), _lattice(rows, n), True
    # ---- shapes whose k-d halves are wholly collinear
    for n in (5, 16, 33, 120):
        row, col = np.stack([np.arange(n) * STEP, np.full(n, (n // 2) * STEP)], 1), np.stack([np.full(n, (n // 2) * STEP), np.arange(n) * STEP], 1)
        yield "halves_cross_%d" % n, np.concatenate([row, col[col[:, 1] != (n // 2) * STEP]]), True
        yield "halves_L_%d" % n, np.concatenate([np.stack([np.arange(n) * STEP, np.zeros(n, int)], 1), np.stack([np.zeros(n - 1, int), np.arange(1, n) * STEP], 1)]), True
        yield "halves_T_%d" % n, np.concatenate([np.stack([np.arange(n) * STEP, np.zeros(n, int)], 1), np.stack([np.full(n - 1, (n // 2) * STEP), np.arange(1, n) * STEP], 1)]), True
        yield "halves_row_far_col_%d" % n, np.concatenate([np.stack([np.arange(n) * STEP, np.zeros(n, int)], 1), np.stack([np.full(n, 4000), np.arange(n) * STEP + 50], 1)]), True
        teeth = np.concatenate([np.stack([np.full(4, x), np.arange(1, 5) * STEP], 1) for x in np.arange(0, n, 4) * STEP])
        yield "halves_comb_%d" % n, np.concatenate([np.stack([np.arange(n) * STEP, np.zeros(n, int)], 1), teeth]), True
    # ---- complete lattices: every quadruple co-circular, the order of ties alone decides
    shapes = [(3, 3), (8, 8), (2, 50), (50, 2), (63, 63), (80, 50), (69, 58), (64, 64), (65, 63), (241, 17), (64, 60)] + CUT_LATTICES
    for w, h in shapes:
        yield "lattice_%dx%d" % (w, h), _lattice(w, h, 5, 5), True
    yield "lattice_kitti_%dx%d" % KITTI_GRID, _lattice(*KITTI_GRID), True
    yield "lattice_4k_%dx%d" % GRID_4K, _lattice(*GRID_4K), False
    # ---- extremes of the admitted coordinate box: co-circular and nearly co-circular quadruples whose in-circle terms are as large
    # as they get (a predicate evaluated in floating point, or in too few bits, flips here)
    block = _lattice(3, 3, 3580, 2040)
    corners = [(X_MIN, 0), (X_MAX - 10, 0), (X_MIN, Y_MAX - 10), (X_MAX - 10, Y_MAX - 10)]
    for k, (x, y) in enumerate(corners):
        rect = _arr([[x, y], [x + 10, y], [x, y + 10], [x + 10, y + 10]])
        yield "extreme_rect_corner_%d" % k, rect, False
        for j in range(4):
            for dx, dy in ((STEP, 0), (0, STEP)):
                near = rect.copy()
                near[j] += [dx if j % 2 else -dx, dy if j >= 2 else -dy]
                if X_MIN <= near[j, 0] <= X_MAX and 0 <= near[j, 1] <= Y_MAX:
                    yield "extreme_near_rect_corner_%d_%d_%s" % (k, j, "x" if dx else "y"), near, False
    yield "extreme_rects_all_corners", np.concatenate([_arr([[x, y], [x + 10, y], [x, y + 10], [x + 10, y + 10]]) for x, y in corners]), False
    # isosceles trapezoids on the whole box: (X_MIN, 0), (X_MAX, 0), (X_MAX - k, Y_MAX), (X_MIN + k, Y_MAX) are co-circular for every k
    # (in-circle determinant 0 with terms near 2^57); moving one corner by one unit gives the smallest nonzero determinants there are at
    # this size.  (Its value is always even for integer points - the lifted coordinate x^2 + y^2 has the parity of x + y - so +-1
    # itself cannot occur: +-2 on the unit square below is the smallest.)
    for k in (0, 5, 2000, 4606):
        trap = _arr([[X_MIN, 0], [X_MAX, 0], [X_MAX - k, Y_MAX], [X_MIN + k, Y_MAX]])
        yield "extreme_trapezoid_%d" % k, trap, False
        yield "extreme_trapezoid_%d_block" % k, np.concatenate([trap, block]), False
        for j, (corner, dx, dy) in enumerate(((2, -1, 0), (3, 1, 0), (2, 0, -1), (0, 0, 1))):
            near = trap.copy()
            near[corner] += [dx, dy]
            yield "extreme_near_trapezoid_%d_%d" % (k, j), near, False
            yield "extreme_near_trapezoid_%d_%d_block" % (k, j), np.concatenate([near, block]), False
    for k, (x, y) in enumerate([(X_MIN, 0), (X_MAX - 2, Y_MAX - 2)]):
        sq = _arr([[x, y], [x + 1, y], [x, y + 1], [x + 1, y + 1]])
        yield "extreme_unit_square_%d" % k, sq, False
        yield "extreme_unit_square_%d_det2" % k, np.concatenate([sq, _arr([[x + 2, y + 1]])]), False
        yield "extreme_unit_square_%d_det2_far" % k, np.concatenate([sq, _arr([[x + 2, y + 1], [X_MAX - x + X_MIN, Y_MAX - y]])]), False


def _seed(name):
    return zlib.crc32(name.encode())


def sets(max_points=None):
    """(name, xy int32) of the whole corpus; max_points leaves the larger sets out (the callers that use it say which)."""
    for name, p, right in _families():
        p = np.ascontiguousarray(p, dtype=np.int32)
        variants = [(name, p)]
        if right:
            q = p.copy()
            q[:, 0] -= int(p[:, 0].min()) - (X_MIN if int(np.ptp(p[:, 0])) <= X_MAX - X_MIN - 200 else -195)
            variants.append((name + "_negx", q))
        for vname, v in variants:
            if max_points is not None and len(v) > max_points:
                continue
            yield vname, v
            yield vname + "_shuffled", np.ascontiguousarray(v[np.random.default_rng(_seed(vname)).permutation(len(v))])


def is_collinear(xy):
    u = np.unique(np.asarray(xy, dtype=np.int64), axis=0)
    if len(u) < 3:
        return True
    d = u - u[0]
    return bool(np.all(d[:, 0] * d[1, 1] == d[:, 1] * d[1, 0]))


def kd_order_coordinates(xy):
    """Plain restatement of what the triangulation's preparation leaves (triangle.cpp:5183-5360, 5889-5903), as coordinates: the distinct
    points, cut alternately by x and by y at n >> 1 down to groups of two or three, which are in (x, y) order."""
    u = np.unique(np.asarray(xy, dtype=np.int64), axis=0)  # sorted by (x, y)

    def rec(p, axis):
        n = len(p)
        if n <= 3:
            return [p[np.lexsort((p[:, 1], p[:, 0]))]]
        o = np.lexsort((p[:, 1], p[:, 0])) if axis == 0 else np.lexsort((p[:, 0], p[:, 1]))
        p = p[o]
        return rec(p[: n >> 1], axis ^ 1) + rec(p[n >> 1:], axis ^ 1)

    return np.concatenate(rec(u, 0)) if len(u) else u


# ---- image pairs with a degenerate support set -------------------------------------------------------------------------------------

def _texture(h, w, seed):
    """Strong, unambiguous texture: fixed-seed noise, smoothed a little so that the Sobel descriptors are not pure noise."""
    a = np.random.default_rng(seed).integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    b = (a[:-2, 1:-1] + a[2:, 1:-1] + a[1:-1, :-2] + a[1:-1, 2:] + 4 * a[1:-1, 1:-1]) / 8.0
    return np.clip(np.rint(b), 0, 255).astype(np.uint8)


def _shift_right(L, disp):
    """Right image of `L` for a per-column disparity (R(u - d) = L(u)); columns nothing maps to keep L's value."""
    R = L.copy()
    h, w = L.shape
    for u in range(w):
        t = u - int(disp[u])
        if 0 <= t < w:
            R[:, t] = L[:, u]
    return R


def _params(cls, disp_max, **kw):
    p = cls.preset("robotics")
    p.disp_max = disp_max
    p.add_corners = 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def pair_cases():
    """(name, kind, H, W, parameter overrides): kind "row" / "col" = one textured band on a lattice row / column of a flat image;
    "lattice" = a complete support lattice (texture everywhere right of a flat margin, inconsistency filter off; the redundancy filter
    has no switch, so the disparity rises by 2 from lattice cell to lattice cell in both directions and no point has an equal
    neighbour; lattice step 10 so that a point's 7 x 7 descriptor window lies inside its own cell); "strip" = two adjacent lattice rows
    at the smallest admitted height (the compiled reference does not survive 32 rows - see test_small_and_odd_image_sizes - the
    restatement does and defines the result there)."""
    return [
        ("band_row_320x120", "row", 120, 320, {}),
        ("band_row_203x97", "row", 97, 203, {}),
        ("band_row_sub_320x120", "row", 120, 320, {"subsampling": 1}),
        ("band_col_320x120", "col", 120, 320, {}),
        ("band_col_161x140", "col", 140, 161, {}),
        ("full_lattice_170x90", "lattice", 90, 170, {"incon_window_size": 0, "incon_min_support": 0, "candidate_stepsize": 10, "disp_max": 63}),
        ("strip_two_rows_240x32", "strip", 32, 240, {"incon_window_size": 0, "incon_min_support": 0}),
    ]


def make_pair(name):
    """(L, R, disp_max, overrides) of one of pair_cases()."""
    case = {c[0]: c for c in pair_cases()}[name]
    _, kind, H, W, over = case
    D = 32
    L = np.full((H, W), 128, np.uint8)
    if kind == "row":
        # a band of 3 image rows on lattice row v: the descriptor of a lattice point reads gradients of rows v - 2 .. v + 2, each from
        # rows +- 1, so texture within 3 rows of v reaches no other lattice row (v +- 5).  The disparity steps along the band so that the
        # redundancy filter (equal neighbours on both sides within 5 lattice cells) keeps points.
        v = 60 if H >= 120 else 40
        L[v - 1:v + 2] = _texture(3, W, _seed(name))
        disp = 4 + (np.arange(W) // 25) % 2 * 6 + (np.arange(W) // 50) * 2
        R = np.full((H, W), 128, np.uint8)
        R[v - 1:v + 2] = _shift_right(L[v - 1:v + 2], disp)
        return L, R, D - 1, over
    if kind == "col":
        u = 160 if W >= 320 else 80
        L[:, u - 1:u + 2] = _texture(H, 3, _seed(name))
        R = np.full((H, W), 128, np.uint8)
        # the disparity changes down the band: every block of 25 image rows has its own
        for r0 in range(0, H, 25):
            d = 5 + (r0 // 25) % 3 * 4
            R[r0:r0 + 25, u - 1 - d:u + 2 - d] = L[r0:r0 + 25, u - 1:u + 2]
        return L, R, D - 1, over
    if kind == "lattice":
        step, half, margin = 10, 5, 45
        L, R = _texture(H, W, _seed(name)), _texture(H, W, _seed(name) + 1)
        L[:, :margin] = R[:, :margin] = 128  # (no support left of the margin: there u - d would leave the image)
        for vi in range(1, H // step + 1):
            for ui in range(margin // step + 1, W // step + 1):
                u, v, d = ui * step, vi * step, 2 * ui + 2 * vi
                if u + half <= W and v + half <= H:
                    R[v - half:v + half, u - half - d:u + half - d] = L[v - half:v + half, u - half:u + half]
        return L, R, over["disp_max"], over
    if kind == "strip":
        # texture on image rows 9 .. 16 reaches the lattice rows 10 and 15 and no other (see "row")
        L[9:17] = _texture(8, W, _seed(name))
        R = np.full((H, W), 128, np.uint8)
        R[9:17] = _shift_right(L[9:17], 3 + (np.arange(W) // 40) * 2)
        return L, R, D - 1, over
    raise ValueError(kind)


def pair_params(cls, name):
    """ROBOTICS with add_corners = 0 plus the case's overrides, as `cls` (ElasParams or SvParams)."""
    _, _, disp_max, over = make_pair(name)
    return _params(cls, disp_max, **{k: v for k, v in over.items() if k != "disp_max"})
