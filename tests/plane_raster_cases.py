"""Support lattices painted point by point for the middle block of the disparity engine - k_grid_mark and k_grid_dilate (K3), k_planes with
solve3 (K4), k_raster_tiles and the plane-dependent half of k_dense in csrc/kernels.hip - and a plain numpy restatement of what they do.

A case is an int16 [Hc][Wc] lattice under the sv_debug_inject_lattice contract (-1 or 0 .. disp_max, lattice row 0 and column 0 zero), the
image size, the preset and the parameter overrides it runs with, and a note of what it is aimed at.  Every case runs with
incon_min_support = 0, so that the consistency filter keeps everything, and keeps painted neighbours within five lattice steps at least
2 apart, so that the redundancy passes keep everything: the support list is the painted set (plus the corner points with add_corners).
The expected stages come from the oracle (orc_planes, orc_grid, orc_raster, orc_dense behind orc_support_filter and orc_delaunay).

The restatement covers the grid marking and flat dilation, the plane-validity rule, the tile binning footprint of k_planes and the scan
conversion (float32 products and sums rounded one by one, truncation toward zero, the last triangle in list order wins).  Each part
takes the name of ONE mistake a rewrite would plausibly make (`bug`): with bug=None it is the oracle, with the mistakes a case names it
is not - tests/test_plane_raster_edges.py asserts both on the CPU and compares the kernels with the oracle on the GPU.

Two mistakes one would like to show cannot change any result (SILENT): the same test asserts that too, and says why."""
import numpy as np

import lattice_cases as lc

# restated from csrc/kernels.hip (the tests read the file and compare)
RT_W, RT_H, RT_CAP = 64, 32, 512   # raster tiles and the length of a tile's triangle list
LANES = 8                          # lanes per triangle in k_raster_tiles: columns of a triangle taken per trip
VALID = 0.7                        # a plane slope at or beyond it switches the prior off (elas.cpp:910)
MASK_WORDS = 8                     # DENSE_MASK_WORDS: mask words of a grid cell k_dense keeps in registers
GRID = 20                          # grid_size of every preset

BUGS = ("b_exclusive", "first_wins", "row_inclusive", "tile_clip", "float_valid", "same_side_d", "row_dilation", "trunc_cell", "no_clamp")
# floor_edge: floor instead of truncation on a negative edge value.  An edge line is evaluated between its end points only, whose rows are
#   0 or more: a negative value is a rounding residue above -1, and both -1 and 0 are clipped to row 0 as the lower end of a column piece
#   and leave it empty as the upper end.  (Unclipped, floor would ask for row -1: scan() counts such rows in info["outside"].)
# le_valid: `<= 0.7` for `< 0.7`.  The slope is a float and 0.7 is none: compared in double no slope equals it, and compared in float
#   `<= 0.7f` is `< 0.7` in double.  The mistake that does show at a slope of exactly -0.7f is the comparison `< 0.7f` in float: float_valid.
SILENT = ("floor_edge", "le_valid")


def params(cls, case):
    """The parameters of a case as `cls` (ElasParams or SvParams)."""
    p = cls.driver(case.disp_max) if case.preset == "driver" else cls.preset(case.preset)
    p.disp_max = case.disp_max
    for k, v in case.over.items():
        setattr(p, k, v)
    return p


class Case:
    def __init__(self, name, family, lattice, image, over, aim, bugs, step=5, preset="driver", disp_max=255, rt_caps=(), expect=None):
        self.name, self.family, self.aim, self.step, self.preset, self.disp_max = name, family, aim, step, preset, disp_max
        self.over = dict(incon_min_support=0, add_corners=0)
        self.over.update(over)
        self.lattice = np.ascontiguousarray(lattice, np.int16)
        self.lattice.setflags(write=False)
        self.Hc, self.Wc = self.lattice.shape
        self.W, self.H = image
        assert ((self.W + step - 1) // step, (self.H + step - 1) // step) == (self.Wc, self.Hc), name
        self.bugs, self.rt_caps, self.expect = tuple(bugs), tuple(rt_caps), dict(expect or {})
        self.sub = int(self.over.get("subsampling", 0))
        self.add_corners = int(self.over["add_corners"])

    def key(self):
        """Cases of one key share a handle: one image size, one preset, one parameter set."""
        return (self.W, self.H, self.preset, self.disp_max, tuple(sorted(self.over.items())))

    def painted(self):
        """The list the filters must leave: the painted points in collection order, plus the corner points."""
        return lc.collect(self.lattice.astype(np.int32), self.step, self.W, self.H, self.add_corners)[0]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
F = np.float32


def grid_dims(W, H, disp_max):
    return disp_max + 2, -(-W // GRID), -(-H // GRID)


def grid(sup, W, H, disp_max, right, bug=None):
    """elas.cpp:577-653 -> int32 [gh][gw][disp_max + 2] (count, then the candidates in ascending order), the oracle's layout.
    Marking: the support disparity and its two neighbours within 0 .. disp_max, in the cell of (u, v) - of (u - d, v) for the right image,
    and no cell where that column is negative (floor, not truncation).  Dilation: 3 x 3 over the FLAT cell array, for the cells
    gw + 1 .. ncell - gw - 2: it wraps at the row ends and leaves the first and last cell row (and two more cells) empty."""
    _, gw, gh = grid_dims(W, H, disp_max)
    D, ncell = disp_max + 1, gw * gh
    flat = np.zeros(ncell * D, bool)   # (the reference's array: cell-major, one flag per disparity)
    for u, v, d in np.asarray(sup, np.int64):
        if right:
            q = F(u - d) / F(GRID)
            x = int(np.trunc(q)) if bug == "trunc_cell" else int(np.floor(q))
        else:
            x = int(u) // GRID
        y = int(np.floor(F(v) / F(GRID)))
        if not (0 <= x < gw and 0 <= y < gh):
            continue
        lo, hi = (d - 1, d + 1) if bug == "no_clamp" else (max(d - 1, 0), min(d + 1, disp_max))
        for dd in range(lo, hi + 1):   # (unclamped, -1 and disp_max + 1 land in the neighbouring cell of the flat array)
            i = (y * gw + x) * D + dd
            if 0 <= i < flat.size:
                flat[i] = True
    cells = flat.reshape(gh, gw, D)
    out = np.zeros((ncell, D), bool)
    if bug == "row_dilation":   # a 3 x 3 window per cell row that stops at the row's ends
        pad = np.zeros((gh + 2, gw + 2, D), bool)
        pad[1:-1, 1:-1] = cells
        acc = np.zeros((gh, gw, D), bool)
        for dy in range(3):
            for dx in range(3):
                acc |= pad[dy:dy + gh, dx:dx + gw]
        acc[0] = acc[-1] = False
        out = acc.reshape(ncell, D)
    else:
        src = flat.reshape(ncell, D)
        for c in range(gw + 1, ncell - gw - 1):
            out[c] = np.any([src[c + dy * gw + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    res = np.zeros((ncell, disp_max + 2), np.int32)
    for c in range(ncell):
        ds = np.flatnonzero(out[c])
        res[c, 0] = len(ds)
        res[c, 1:1 + len(ds)] = ds
    return res.reshape(gh, gw, disp_max + 2)


def planes(sup, tri):
    """elas.cpp:503-575 by Cramer's rule on the integer corners: ([nt][6] float32 t1a t1b t1c t2a t2b t2c, [nt][2] singular).
    (The determinants are exact in double, the quotients rounded once; the reference's Gauss-Jordan steps may differ from that in the
    last bits of the double - the float it is rounded to is compared with a tolerance of one unit in the last place.)
    A triangle of one image may have its corners on one line in the OTHER image: that system is singular, its planes here are 0.  The
    reference does not notice (its pivot test is 1e-20, the elimination leaves a residue of 1e-16) and divides by the residue: what it
    stores then - slopes of 1e15 - is no plane, but it is what plane_d is compared with, and the kernels must store the same bits."""
    sup = np.asarray(sup, np.int64)
    out = np.zeros((len(tri), 6), np.float32)
    singular = np.zeros((len(tri), 2), bool)
    for i, t in enumerate(np.asarray(tri)):
        u, v, d = sup[t, 0], sup[t, 1], sup[t, 2]
        for side in (0, 1):
            x = u - side * d
            det = int(x[0] * (v[1] - v[2]) - v[0] * (x[1] - x[2]) + (x[1] * v[2] - x[2] * v[1]))
            if det == 0:
                singular[i, side] = True
                continue
            a = int(d[0] * (v[1] - v[2]) - v[0] * (d[1] - d[2]) + (d[1] * v[2] - d[2] * v[1]))
            b = int(x[0] * (d[1] - d[2]) - d[0] * (x[1] - x[2]) + (x[1] * d[2] - x[2] * d[1]))
            c = int(x[0] * (v[1] * d[2] - v[2] * d[1]) - v[0] * (x[1] * d[2] - x[2] * d[1]) + d[0] * (x[1] * v[2] - x[2] * v[1]))
            out[i, 3 * side:3 * side + 3] = (a / det, b / det, c / det)
    return out, singular


def valid(pl, right, bug=None):
    """elas.cpp:910: the prior counts for a triangle only where |plane_a| < 0.7 and |plane_d| < 0.7 - plane_a this image's slope in u,
    plane_d the OTHER image's, both floats, compared in double."""
    pl = np.asarray(pl, np.float32).reshape(-1, 6)
    a, d = (pl[:, 3], pl[:, 0]) if right else (pl[:, 0], pl[:, 3])
    if bug == "same_side_d":
        d = a
    if bug == "float_valid":
        return (np.abs(a) < F(VALID)) & (np.abs(d) < F(VALID))
    if bug == "le_valid":
        return (np.abs(a).astype(np.float64) <= VALID) & (np.abs(d).astype(np.float64) <= VALID)
    return (np.abs(a).astype(np.float64) < VALID) & (np.abs(d).astype(np.float64) < VALID)


def corners(sup, t, right):
    """elas.cpp:859-884: the corners (u, v) as floats, sorted by u with the reference's three compare-and-swap steps.  Returns
    (A, B, C, swapped)."""
    tu = [F(sup[k][0] - sup[k][2]) if right else F(sup[k][0]) for k in t]
    tv = [F(sup[k][1]) for k in t]
    swapped = False
    for j in range(3):
        for k in range(j):
            if tu[k] > tu[j]:
                tu[j], tu[k] = tu[k], tu[j]
                tv[j], tv[k] = tv[k], tv[j]
                swapped = True
    return (tu[0], tv[0]), (tu[1], tv[1]), (tu[2], tv[2]), swapped


def edges(A, B, C):
    """elas.cpp:887-906: the columns (int)A_u, (int)B_u, (int)C_u and slope and offset of AC, AB, BC; a slope stays 0 where the two
    columns are equal."""
    (A_u, A_v), (B_u, B_v), (C_u, C_v) = A, B, C
    a_u, b_u, c_u = int(A_u), int(B_u), int(C_u)
    AB_a = (A_v - B_v) / (A_u - B_u) if a_u != b_u else F(0)
    AC_a = (A_v - C_v) / (A_u - C_u) if a_u != c_u else F(0)
    BC_a = (B_v - C_v) / (B_u - C_u) if b_u != c_u else F(0)
    return (a_u, b_u, c_u), (AC_a, A_v - AC_a * A_u), (AB_a, A_v - AB_a * A_u), (BC_a, B_v - BC_a * B_u)


def scan(sup, tri, W, H, right, bug=None, info=None):
    """elas.cpp:912-940 -> int32 [H][W]: per triangle in list order the columns max(A_u, 0) .. min(C_u, W) - 1, with the edge AB left of
    B_u and BC from B_u on against the long edge AC; per column the rows min(v_1, v_2) .. max(v_1, v_2) - 1 within the image.  A later
    triangle overwrites an earlier one.  info: a dict that receives "boxes" ([nt][4] u0, u1, v0, v1 of the pixels written, -1 where
    none), "outside" (rows asked for outside the image before the clip) and "trips" (the most 8-lane trips a triangle's columns take)."""
    sup = np.asarray(sup, np.int64)
    ids = np.full((H, W), -1, np.int32)
    rows = np.arange(H, dtype=np.int64)[:, None]
    boxes = np.full((len(tri), 4), -1, np.int64)
    outside = trips = 0
    cut = np.floor if bug == "floor_edge" else np.trunc
    for i, t in enumerate(np.asarray(tri)):
        A, B, C, _ = corners(sup, t, right)
        (a_u, b_u, c_u), (AC_a, AC_b), (AB_a, AB_b), (BC_a, BC_b) = edges(A, B, C)
        us = np.arange(max(a_u, 0), min(c_u, W))
        if us.size == 0:
            continue
        trips = max(trips, -(-us.size // LANES))
        uf = us.astype(np.float32)
        second = us > b_u if bug == "b_exclusive" else us >= b_u
        e_a, e_b = np.where(second, BC_a, AB_a).astype(np.float32), np.where(second, BC_b, AB_b).astype(np.float32)
        v1 = cut(F(AC_a) * uf + F(AC_b)).astype(np.int64)   # (a float32 product, then a float32 sum: no fused multiply-add)
        v2 = cut(e_a * uf + e_b).astype(np.int64)
        lo, hi = np.minimum(v1, v2), np.maximum(v1, v2) + (1 if bug == "row_inclusive" else 0)
        lo_c, hi_c = np.clip(lo, 0, H), np.clip(hi, 0, H)
        outside += int(((hi - lo) - np.maximum(hi_c - lo_c, 0)).sum()) if bug != "row_inclusive" else 0
        full = hi_c > lo_c
        if not full.any():
            continue
        r0, r1 = int(lo_c[full].min()), int(hi_c[full].max())
        m = (rows[r0:r1] >= lo_c) & (rows[r0:r1] < hi_c)
        if bug == "tile_clip":   # a tile that ends one column early
            m &= (us % RT_W != RT_W - 1)[None, :]
        view = ids[r0:r1, us[0]:us[-1] + 1]
        if bug == "first_wins":
            m &= view == -1
        view[m] = i
        boxes[i] = (us[full].min(), us[full].max(), r0, r1 - 1)
    if info is not None:
        info.update(boxes=boxes, outside=outside, trips=trips)
    return ids


def footprints(sup, tri, W, H, right):
    """k_planes' tile binning: [nt][4] u_begin, u_end, v_begin, v_end (half open; empty where begin >= end) - the columns
    max(A_u, 0) .. min(C_u, W) and the rows of the corners widened by one above and two below for the truncations."""
    sup = np.asarray(sup, np.int64)
    out = np.zeros((len(tri), 4), np.int64)
    for i, t in enumerate(np.asarray(tri)):
        A, B, C, _ = corners(sup, t, right)
        vs = (A[1], B[1], C[1])
        out[i] = (max(int(A[0]), 0), min(int(C[0]), W), max(int(min(vs)) - 1, 0), min(int(max(vs)) + 2, H))
    return out


def tile_counts(fp, W, H):
    """Triangles binned per raster tile, [tile rows][tile columns]."""
    ntx, nty = -(-W // RT_W), -(-H // RT_H)
    cnt = np.zeros((nty, ntx), np.int64)
    for ub, ue, vb, ve in fp:
        if ub < ue and vb < ve:
            cnt[vb // RT_H:(ve - 1) // RT_H + 1, ub // RT_W:(ue - 1) // RT_W + 1] += 1
    return cnt


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
CASES, FAMILIES = {}, {}
IMG = (320, 120)


def _add(name, family, pts, aim, bugs, image=IMG, over=None, step=5, **kw):
    """pts: (lattice column, lattice row, disparity) of every painted point."""
    assert name not in CASES
    W, H = image
    d = lc.blank(-(-W // step), -(-H // step))
    for k, j, x in pts:
        assert k >= 1 and j >= 1 and d[j, k] == -1 and 0 <= x <= kw.get("disp_max", 255), (name, k, j, x)
        d[j, k] = x
    CASES[name] = Case(name, family, d, image, over or {}, aim, bugs, step=step, **kw)
    FAMILIES.setdefault(family, []).append(name)


def _every_second(fn, Wc=64, Hc=24, hi=255):
    """fn(k, j) on every second lattice node - k, j count the painted columns and rows, 10 pixels apart at step 5 - where it is a disparity."""
    return [(2 * k, 2 * j, fn(k, j)) for k in range(1, (Wc + 1) // 2) for j in range(1, (Hc + 1) // 2) if 0 <= fn(k, j) <= hi]


# slopes.  d = 230 - s k + 2 j: t1a = -s / 10, t1b = 0.2; the right image's slope t2a = t1a / (1 - t1a).
for _s, _what, _bugs, _x in ((6, "-0.6: every triangle valid on both sides", ("b_exclusive", "trunc_cell"), dict(t1a=-0.6, valid=(1, 1))),
                             (7, "-0.7f: valid in double, not in float", ("float_valid", "row_inclusive"), dict(t1a=-0.7, valid=(1, 1))),
                             (8, "-0.8: invalid on the left by its own slope, on the right by the other side's alone (t2a = -0.44)", ("same_side_d",), dict(t1a=-0.8, valid=(0, 0)))):
    _add("slope_m0%d" % _s, "slopes", _every_second(lambda k, j: 230 - _s * k + 2 * j), "left-plane slope " + _what, _bugs, expect=_x)
_add("slope_p04", "slopes", _every_second(lambda k, j: 10 + 4 * k + 2 * j), "slope 0.4: t2a = 0.667, valid on both sides", ("b_exclusive", "row_inclusive"), expect=dict(t1a=0.4, valid=(1, 1)))
_add("slope_p05", "slopes", _every_second(lambda k, j: 10 + 5 * k + 2 * j), "slope 0.5: t2a = 1.0, invalid on the left by the other side's slope alone", ("same_side_d",),
     expect=dict(t1a=0.5, valid=(0, 0)))
_add("slope_const", "slopes", [(6 * k, 6 * j, 40) for k in range(1, 11) for j in range(1, 4)], "a constant plane on points six lattice steps apart: every slope exactly 0", ("b_exclusive",),
     expect=dict(t1a=0.0, valid=(1, 1)))
_add("slope_v_only", "slopes", _every_second(lambda k, j: 20 + 9 * j + 2 * (k % 3)), "a slope in v only (0.9) under a ripple of 2 and 4 in u", ("row_inclusive", "first_wins"))

# folds: disparity steps larger than the point spacing - u - d is not monotone in u, the right image's triangulation is another one
# (2 per column inside a block and spacing - 2 per row: the points (k, j) and (k + 1, j + 1) of a block share their right-image column)
_fold = lambda spacing: lambda k, j: 40 + 65 * ((k // 4) % 2) + (spacing - 2) * j + 2 * (k % 4)
_add("fold_blocks", "folds", _every_second(_fold(10)), "blocks of four columns that jump by 65: the right image's columns interleave, corner order reverses", ("b_exclusive", "tile_clip"),
     expect=dict(folds=True))
_add("fold_teeth", "folds", _every_second(lambda k, j: 30 + 23 * (k % 3) + 2 * j + 10 * (j % 2) * (k % 2)), "teeth of 23 over points 10 apart: every third column falls behind its neighbours",
     ("row_inclusive", "first_wins"), expect=dict(folds="swap"))

# negative columns: d > u at the left of the lattice
_add("neg_columns", "negative", _every_second(lambda k, j: 60 + 3 * k + 2 * j), "u - d = 7 k - 60 - 2 j: right-image triangles left of column 0 and across it, support points in -20 .. -1",
     ("trunc_cell", "b_exclusive"), expect=dict(negative=True))
_add("neg_corners", "negative", [(2, 2, 70), (4, 4, 31), (3, 7, 33), (9, 3, 52), (12, 12, 58), (30, 20, 9)], "the same with corner points that copy a large disparity: long edges from far left of the image",
     ("trunc_cell", "same_side_d"), over=dict(add_corners=1), expect=dict(negative=True))

# sparse sets
_add("sparse_three", "sparse", [(10, 4, 12), (50, 9, 90), (23, 21, 47)], "exactly three painted points: one triangle per side", ("row_inclusive", "tile_clip"), expect=dict(n=3, nt=(1, 1)))
_add("sparse_corners_only", "sparse", [], "no painted point: the six corner points (two of them twice) - triangles larger than a tile, 40 trips of eight lanes", ("tile_clip", "row_inclusive"),
     over=dict(add_corners=1), expect=dict(n=6, big=True))
_add("sparse_corners_one", "sparse", [(31, 11, 200)], "one painted point of disparity 200 that all corners copy: right-image edges from column -200", ("tile_clip", "row_inclusive"),
     over=dict(add_corners=1), expect=dict(n=7, big=True, far_left=-200))

# seams of the 64 x 32 raster tiles
_add("seam_rows", "seams", [(k, 32, 20 + 4 * (k % 7) + k // 7) for k in range(2, 63, 2)] + [(12, j, 90 + 3 * j) for j in range(2, 31, 2)] + [(13, j, 150 + 3 * j) for j in range(3, 32, 2)] +
     [(40, 10, 15), (55, 20, 25)],
     "320 x 170: a lattice row at v = 160 = 5 x 32 and points at u = 60 and 65 around the seam at 64", ("tile_clip", "b_exclusive"), image=(320, 170), expect=dict(seam=True, singular=True))
for _W, _H in ((64, 32), (65, 33)):
    _add("seam_%dx%d" % (_W, _H), "seams", [(3, 2, 14), (9, 4, 22), (6, 5, 9), (11, 1, 30)], "%d x %d: %s" % (_W, _H, "exactly one tile" if _W == 64 else "one tile and one pixel more each way"),
         ("tile_clip", "b_exclusive"), image=(_W, _H), over=dict(add_corners=1))

# tile lists.  rt_caps: the values of sv_debug_set "rt_cap" the case runs with on top of the handle's own (None here); "tile": the count
# of the tile the test picks so that tiles below, at and above it exist
_FULL = [(k, j, (2 * k + 12 * j) % 240) for k in range(1, 64) for j in range(1, 24)]
_add("tiles_full", "tiles", _FULL, "every lattice point painted: tile lists below, at and above a cap chosen from the binning counts; caps 0 and 1", ("tile_clip", "first_wins"),
     rt_caps=("tile", 0, 1), expect=dict(n=63 * 23))
# (at step 2 a disparity that rises by 2 per lattice column is a slope of exactly 1: d = (2 k + 12 j) mod 240 would put a whole lattice row
# on ONE right-image vertex.  A sawtooth of 4 per column over six columns, and of 2 per row over six rows, keeps neighbours within five
# steps apart, every u - d of a row distinct, and both images' triangulations inside the image)
_add("tiles_real_cap", "tiles", [(k, j, 10 + 4 * (k % 6) + 2 * (j % 6)) for k in range(1, 65) for j in range(1, 33)],
     "130 x 66 at step 2, every lattice point painted: about a thousand triangles per tile, past the real cap of 512 with no debug knob", ("tile_clip", "b_exclusive"),
     image=(130, 66), step=2, over=dict(candidate_stepsize=2), expect=dict(n=64 * 32, over_cap=True))

# mask words: support disparities at the ends of the 32-bit words of a cell's mask and at 0 and disp_max, for every width of the mask
_WORD_EDGES = (0, 1, 30, 31, 32, 33, 62, 63, 64)
for _dm in (63, 95, 127, 191, 255, 287):
    _vals = sorted({x for x in _WORD_EDGES + (_dm - 1, _dm) + tuple(range(95, _dm, 32)) + tuple(range(96, _dm, 32)) if x <= _dm})
    _nodes = [(6 * k, 6 * j) for j in range(1, 4) for k in range(1, 11)]
    assert len(_vals) <= len(_nodes)
    _pts = [(k, j, _vals[i % len(_vals)]) for i, (k, j) in enumerate(_nodes)]
    for _preset in ("driver", "robotics"):
        _add("words_%s_d%d" % (_preset, _dm), "words", _pts, "disp_max %d: %d mask words, %s" % (_dm, (_dm + 32) // 32, "plane radius 3" if _preset == "driver" else "plane radius 2, match_texture 1"),
             ("no_clamp", "row_inclusive"), preset=_preset, disp_max=_dm, expect=dict(values=_vals))

# dilation over the flat cell array
_add("dilate_last_column", "dilation", [(61, 7, 207), (62, 9, 209), (63, 11, 211), (8, 8, 40), (20, 15, 60), (30, 5, 80)],
     "a cluster in the last grid column only, of disparities nothing else has: the flat dilation carries it into column 0 of the rows below", ("row_dilation", "b_exclusive"),
     expect=dict(wrap=(206, 212)))
_add("dilate_end_rows", "dilation", [(10, 1, 100), (30, 3, 104), (50, 2, 108), (12, 22, 150), (33, 23, 154), (52, 21, 158), (25, 12, 20)],
     "points in the first and the last grid row: those rows stay empty, their neighbours take the points", ("row_dilation", "row_inclusive"), expect=dict(end_rows=True))
_add("dilate_32x32", "dilation", [(2, 2, 5), (5, 3, 12), (3, 6, 19), (6, 6, 3)], "32 x 32: two grid rows, no cell the dilation writes - every grid is empty", ("first_wins", "b_exclusive"),
     image=(32, 32), over=dict(add_corners=1), expect=dict(empty_grid=True))

# subsampling: an even lattice step (6), half-size maps, tri_id at full resolution
_SUB = dict(subsampling=1)
_add("sub_slope_m07", "subsampling", _every_second(lambda k, j: 230 - 7 * k + 2 * j, 54, 20), "subsampling with points 12 apart: slope -7 / 12", ("b_exclusive", "row_inclusive"), over=_SUB, step=6)
_add("sub_fold_blocks", "subsampling", _every_second(_fold(12), 54, 20), "subsampling on the folded lattice", ("b_exclusive", "row_inclusive"), over=_SUB, step=6, expect=dict(folds=True))
