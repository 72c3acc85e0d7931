"""Seeded cases for the three world-map stages at the points where their BATCH and CAPACITY loops turn over - what the stages' own tests,
which pin the tile edges of the map, never reach.  Pure numpy on top of the definitions in stereo_vision.sv (passed in as `sv`); nothing
here is random beyond the fixed seeds.  tests/test_map_stage_edges.py asserts on the CPU that every case is what it claims to be, and
compares the kernels with the definitions on the GPU.

fuse     FUSE_BATCHES frames around the cull's round of 64 on the two SMALL cases of test_occupancy_map.py: fuse_patterns(B) names the
         frames that touch the map (every other pose is far away or has a word that is not finite), fuse_batch() the poses and runs of
         all-occupied frames followed by all-free ones.  cull_ballots() is the kernel's cull in numpy - the 64-bit set of frames per strip and round -
         and seen_pairs() the (cell, frame) pairs strictly inside the frame's ranges.  fuse_geometries() are the frames, maps and poses
         that stress the cull's margin.
match    MATCH_GRIDS: frame grids of 4095, 4096, 4097, 8193 and 12293 = 3 x 4096 + 5 cells - all of them exact under sv_occupancy_dims'
         rule rows = (x1 - x0) scale + 1 - and the two thinnest grids of 32768 cells in one direction; match_states() per grid;
         candidate_case() a list of three cells whose best candidate stands where the caller puts it.
paths    long_paths(): 65535 steps whose only hit is the last step's last disc, or step 0's disc 0.
cells    check_map_cells(build): the rules the map's readers share are stated once, in csrc/occupancy_map_cells.h and csrc/stage_glue.h."""
import functools
import os
import re

import numpy as np

NAN, INF = float("nan"), float("inf")
INT_MAX = 2 ** 31 - 1
STRIP_ROWS, STRIP_COLS = 2, 32  # a wavefront's strip of the fuse: OCCMAP_WAVE_ROWS x OCCMAP_TILE_COLS

# --------------------------------------------------------------------------------------------------------------- cells

CELLS_HEADER = "occupancy_map_cells.h"
CELLS_KERNELS = ("map_match_kernels.hip", "clearance_kernels.hip", "view_kernels.hip", "frontier_kernels.hip", "occupancy_kernels.hip")
MAP_HOSTS = ("occupancy_map.cpp", "map_match.cpp", "clearance.cpp", "cost.cpp", "frontier.cpp", "view.cpp")
# The texts that define the way of a point into a cell, a cell's state and the line's step: each stands once in csrc/, in the header.
CELLS_TEXTS = ("floor(v * m.ms)",                                        # a world coordinate in cells
               "top - 1 - (int)",                                        # the row of floor(X ms), after the comparisons in double
               "s >= 0 ? (l >= occupied ? 2u : l <= free_ ? 1u : 0u) : 0u",  # the state of a cell
               "(pc * X - ps * Y) + tx",                                 # a vehicle point under a pose
               ">> (16 * (k & 1))",                                      # the wide loader's 16-bit extraction
               "-= two_n")                                               # the line rule's carry
# the same rules whatever the operands are called: no second statement of one under other names
CELLS_SHAPES = (r"floor\(\w+\*[\w.>-]*ms\)", r"top-1-\(int\)", r"\?\(\w+>=[\w.]*occupied\?2u?:", r"\w+\*\w+-\w+\*\w+\)\+\w+,", r"\(\w+>>1\)\]>>\(16\*\(\w+&1\)\)",
                r"-=two_n")


def squeeze(text):
    """Without // comments and without blanks."""
    return re.sub(r"\s+", "", re.sub(r"//.*", "", text))


def check_map_cells(build):
    """The rules that the readers of the flat world map share are defined once, in csrc/occupancy_map_cells.h, and the checks their
    entries share once, in csrc/stage_glue.h.  Returns the squeezed text of the header."""
    assert CELLS_HEADER in build.HEADERS
    names = sorted(n for n in os.listdir(build.CSRC) if n.endswith((".h", ".hip", ".cpp")))
    code = {n: squeeze(open(os.path.join(build.CSRC, n)).read()) for n in names}
    for n in CELLS_KERNELS:
        assert '#include"%s"' % CELLS_HEADER in code[n], n
    for text, shape in zip(CELLS_TEXTS, CELLS_SHAPES):
        for n in names:
            want = 1 if n == CELLS_HEADER else 0
            assert code[n].count(squeeze(text)) == want and len(re.findall(shape, code[n])) == want, (text, n)
    for n in names:
        assert ("rows>32768||cols<1" in code[n]) == (n == "stage_glue.h"), n
    for n in MAP_HOSTS:
        assert "reinterpret_cast<uintptr_t>" not in code[n], n
    return code[CELLS_HEADER]


# ---------------------------------------------------------------------------------------------------------------- fuse

FUSE_BATCHES = (63, 64, 65, 127, 128, 129, 200)
FAR = (1000.0, 0.0, 1.0, 0.0)
FUSE_TOUCHING = {"9x5": [(0.0, 0.0, 1.0, 0.0), (0.555, -0.645, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.3, -0.2, np.cos(0.5), np.sin(0.5))],
                 "41x41": [(0.0, 0.0, 1.0, 0.0), (0.222, -0.258, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0), (0.3, -0.2, np.cos(0.5), np.sin(0.5))]}
FUSE_AWAY = [FAR, (-1000.0, 1e6, 0.6, 0.8), (0.0, NAN, 1.0, 0.0), (INF, 0.0, 1.0, 0.0), (0.0, 0.0, NAN, 0.0), (0.0, 0.0, 1.0, -INF), (1e300, -1e300, 0.0, 1.0)]
# name -> the frames that touch, as a function of B; a pattern without a frame below B is left out for that B (fuse_patterns)
_PATTERNS = {"bit0": lambda B: [0], "bit63": lambda B: [63], "second_round": lambda B: [64], "b63_b64": lambda B: [63, 64], "last": lambda B: [B - 1],
             "all": lambda B: list(range(B)), "none": lambda B: []}


def fuse_patterns(B):
    """name -> sorted list of the frames that touch the map; "mix" is a seeded draw of about half of the frames."""
    out = {}
    for name, fn in _PATTERNS.items():
        at = [b for b in fn(B) if b < B]
        if len(at) == len(fn(B)):
            out[name] = at
    rng = np.random.default_rng(7000 + B)
    out["mix"] = sorted(np.nonzero(rng.random(B) < 0.5)[0].tolist())
    return out


def fuse_batch(case, B, touching, frows, fcols, seed=0):
    """(state uint8 [B, frows, fcols], poses float64 [B, 4]).  Every frame not in `touching` gets one of FUSE_AWAY and random bytes.
    One or two touching frames stand at the case's first pose, so that the ballot is that of one known pose.  More of them draw from
    the case's poses and hold, along the touching frames, five all-occupied frames, fourteen all-free ones and two of random bytes 0 .. 3
    and 255, again and again - with the default words 5 x 85 passes l_max = 350 and 14 x 40 comes down from there past l_min = -200 - and
    the last 24 of them are sixteen all-free frames under the quarter turn followed by eight all-occupied ones under the identity: the
    cells only the quarter turn reaches end at l_min, those under the identity at l_max."""
    rng = np.random.default_rng(seed + 31 * B + len(touching))
    pool = FUSE_TOUCHING[case]
    poses = np.array([FUSE_AWAY[k] for k in rng.integers(0, len(FUSE_AWAY), B)], np.float64).reshape(B, 4)
    state = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), (B, frows, fcols))
    tail = len(touching) - 24 if len(touching) >= 24 else len(touching)
    for j, b in enumerate(touching):
        if len(touching) <= 2:
            poses[b] = pool[0]
        elif j < tail:
            poses[b] = pool[int(rng.integers(0, len(pool)))]
            if j % 21 < 19:
                state[b] = 2 if j % 21 < 5 else 1
        else:
            poses[b], state[b] = (pool[2], 1) if j < tail + 16 else (pool[0], 2)
    return state, poses


def _frame_axes(sv, poses, frame, words, Xw, Yw):
    """(Xf, Yf) float64 [B, len(Xw), len(Yw)] in the kernel's stated arithmetic: two products and a sum per coordinate, each rounded."""
    p = np.asarray(poses, np.float64)
    tx, ty, c, s = (p[:, k][:, None, None] for k in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = Xw[None, :, None] - tx, Yw[None, None, :] - ty
        return c * dx + s * dy, c * dy - s * dx


def seen_pairs(sv, poses, frame, words):
    """The number of (cell, frame) pairs strictly inside the frame's ranges: the lookups no cull may skip."""
    (fx0, fx1), (fy0, fy1), _, _, _ = sv.occupancy_frame_grid(frame)
    Xw, Yw = sv.occupancy_map_centres(words)
    n = 0
    for b0 in range(0, len(poses), 16):  # in slices: the long maps times the batch would not fit otherwise
        Xf, Yf = _frame_axes(sv, poses[b0:b0 + 16], frame, words, Xw, Yw)
        with np.errstate(invalid="ignore"):
            n += int(((Xf > fx0) & (Xf < fx1) & (Yf > fy0) & (Yf < fy1)).sum())
    return n


def cull_ballots(sv, poses, frame, words):
    """uint64 [strips, rounds]: bit k of [s, j] is set iff the cull of occupancy_map_kernels.hip lets frame 64 j + k through for strip s
    (2 rows x 32 columns, row-major over the map) - its arithmetic word for word: the strip's centre carried into the frame's axes,
    the ranges widened by reach * max(1, c^2 + s^2) + cell + 2^-48 (|c dx| + |s dy|)."""
    (fx0, fx1), (fy0, fy1), _, _, _ = sv.occupancy_frame_grid(frame)
    w = sv.occupancy_map_words(words)
    half = 1.0 / (2.0 * float(w["scale"]))
    cell = 2.0 * half
    reach = 0.5 * np.sqrt(float(STRIP_ROWS * STRIP_ROWS + STRIP_COLS * STRIP_COLS)) * cell
    r0 = np.arange(0, w["rows"], STRIP_ROWS, dtype=np.int64)
    c0 = np.arange(0, w["cols"], STRIP_COLS, dtype=np.int64)
    Xc = (2 * w["top"] - (2 * r0 + STRIP_ROWS - 1) - 1).astype(np.float64) * half
    Yc = (2 * w["left"] - (2 * c0 + STRIP_COLS - 1) - 1).astype(np.float64) * half
    p = np.asarray(poses, np.float64)
    B = len(p)
    tx, ty, pc, ps = (p[:, k][:, None, None] for k in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = Xc[None, :, None] - tx, Yc[None, None, :] - ty
        cx, sy, cy, sx = pc * dx, ps * dy, pc * dy, ps * dx
        Xf, Yf = cx + sy, cy - sx
        n = pc * pc + ps * ps
        m = reach * np.where(n > 1.0, n, 1.0) + cell
        mx, my = m + (np.abs(cx) + np.abs(sy)) * 2.0 ** -48, m + (np.abs(cy) + np.abs(sx)) * 2.0 ** -48
        touch = (Xf > fx0 - mx) & (Xf < fx1 + mx) & (Yf > fy0 - my) & (Yf < fy1 + my)
    touch = touch.reshape(B, -1)
    rounds = (B + 63) // 64
    out = np.zeros((touch.shape[1], rounds), np.uint64)
    for b in range(B):
        out[:, b // 64] |= touch[b].astype(np.uint64) << np.uint64(b % 64)
    return out


def fuse_geometries(sv):
    """name -> (frame grid, map words, poses float64 [n, 4]): what stresses the cull's margin.  Every set of poses holds some that touch
    the map and some that do not."""
    base = dict(l_occ=85, l_free=40, l_min=-200, l_max=350)
    hand = dict(x_range=(0, 8), y_range=(-2, 2), scale=1)
    small = dict(base, top=20, left=13, rows=37, cols=29, scale=2)
    turns = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]  # the exact quarter turns
    eighths = [(np.cos(k * np.pi / 4), np.sin(k * np.pi / 4)) for k in (1, 3, 5, 7)]
    out = {}
    # the fewest cells sv_occupancy_dims admits: 2 x 2, far smaller than a wavefront's strip of 2 x 32 map cells
    out["tiny_frame"] = (dict(x_range=(0, 1), y_range=(0, 1), scale=1), small,
                         np.array([(0.0, 0.0, 1.0, 0.0), (3.3, -4.1, 1.0, 0.0), (-7.9, 5.9, 0.0, 1.0), (9.4, -7.2, 0.6, 0.8), (10.1, 0.0, 1.0, 0.0), (0.0, -9.1, 1.0, 0.0), FAR]))
    # a map cell 64 frame cells wide (map scale 1, frame scale 64: 65 x 129 frame cells in 1 m x 2 m), and the reverse
    out["map_cell_x64"] = (dict(x_range=(0, 1), y_range=(-1, 1), scale=64), dict(small, scale=1),
                           np.array([(-0.25, 0.0, 1.0, 0.0), (3.0, -4.0, 0.0, 1.0), (7.3, 2.6, 0.6, -0.8), (-16.9, 0.0, 1.0, 0.0), (21.1, 0.0, 1.0, 0.0), (0.0, -17.6, 1.0, 0.0)]))
    out["frame_cell_x64"] = (hand, dict(small, scale=64, top=64 * 3 + 20, left=13),
                             np.array([(0.0, 0.0, 1.0, 0.0), (3.1, 0.05, 0.0, 1.0), (3.3, 1.9, 0.6, 0.8), (-5.0, 0.0, 1.0, 0.0), (3.0, 2.3, 1.0, 0.0), (3.4, 0.0, 1.0, 0.0), FAR]))
    # borders exactly on cell centres: at scale 2 the centres lie at odd multiples of 0.25, so with t = (0.25, 0.25) and an exact quarter
    # turn whole rows and columns of centres have Xf == 0, Xf == 8, Yf == -2 or Yf == 2 - the comparisons are strict
    out["on_the_border"] = (hand, small, np.array([(0.25, 0.25, c, s) for c, s in turns + eighths] + [(0.25, -0.75, c, s) for c, s in turns] + [FAR]))
    # (c, s) that is no rotation: c^2 + s^2 = 2.5, 13, 0.3125, 0.05, 2e-6
    out["no_rotation"] = (hand, small, np.array([(1.0, 0.5, 1.5, 0.5), (5.0, 1.0, 3.0, -2.0), (1.0, -1.0, 0.5, 0.25), (2.0, 0.0, 0.2, 0.1), (0.0, 0.0, 1e-3, 1e-3), (40.0, 0.0, 3.0, -2.0),
                                                  (-30.0, 5.0, 0.5, 0.25)]))
    # the map at the ends of what check_map admits, the poses moved there
    big = 2 ** 24 - 1
    for name, top, left in (("far_pp", big, big), ("far_mm", -big, -big), ("far_pm", big, -big)):
        x, y = (top - 20) / 2.0, (left - 13) / 2.0  # where SMALL's map has its origin
        out[name] = (hand, dict(small, top=top, left=left),
                     np.array([(x, y, 1.0, 0.0), (x + 0.555, y - 0.645, 1.0, 0.0), (x, y, 0.0, 1.0), (x + 0.3, y - 0.2, np.cos(0.5), np.sin(0.5)), (x + 0.25, y + 0.25, -1.0, 0.0),
                               (x + 19.1, y, 1.0, 0.0), (x, y - 11.0, 1.0, 0.0), (0.0, 0.0, 1.0, 0.0), (-x, -y, 1.0, 0.0)]))
    return out


def geometry_batch(poses):
    """float64 [65, 4]: a geometry's poses again and again, its first two - which touch the map - as frames 63 and 64."""
    many = np.array([poses[(b * 5 + 1) % len(poses)] for b in range(65)])
    many[63], many[64] = poses[0], poses[1]
    return many


MAP_ROWS, MAP_COLS = (1, 7, 8, 9, 17), (1, 31, 32, 33, 65)
LONG_MAPS = ((1, 32768), (32768, 1))


def map_shifts(rows, cols):
    """Shifts that keep part of the map, that keep its last row or column only, and that keep nothing - in either direction."""
    out = [(0, 0), (rows // 2, 0), (-(rows // 3), cols // 2), (0, -(cols // 3)), (rows - 1, 0), (1 - rows, 0), (0, cols - 1), (0, 1 - cols), (rows - 1, 1 - cols),
           (rows, 0), (-rows, 0), (0, cols), (0, -cols - 5), (rows + 40000, 0), (0, -INT_MAX), (INT_MAX, INT_MAX)]
    return sorted(set(out))


def nothing_survives(shift, rows, cols):
    return abs(shift[0]) >= rows or abs(shift[1]) >= cols


# ---------------------------------------------------------------------------------------------------------------- match

# name -> the frame grid; rows x cols = (x1 - x0) scale + 1 times (y1 - y0) scale + 1
MATCH_GRIDS = {"4095": dict(x_range=(0, 31), y_range=(-16, 16), scale=2),        # 63 x 65
               "4096": dict(x_range=(0, 63), y_range=(-31, 32), scale=1),        # 64 x 64
               "4097": dict(x_range=(0, 16), y_range=(-120, 120), scale=1),      # 17 x 241: four staged chunks of 1024 and one entry
               "8193": dict(x_range=(0, 2), y_range=(-1365, 1365), scale=1),     # 3 x 2731
               "12293": dict(x_range=(-9, 9), y_range=(-323, 323), scale=1),     # 19 x 647 = 3 x 4096 + 5
               "long": dict(x_range=(0, 32767), y_range=(0, 1), scale=1),        # 32768 x 2: fr up to 32767
               "wide": dict(x_range=(0, 1), y_range=(0, 32767), scale=1)}        # 2 x 32768: fc << 15 up to 32767 << 15
MATCH_CELLS = {"4095": (63, 65), "4096": (64, 64), "4097": (17, 241), "8193": (3, 2731), "12293": (19, 647), "long": (32768, 2), "wide": (2, 32768)}
MATCH_PAD = 3  # map cells around the frame's points, where 32768 leaves room


def match_map(sv, grid):
    """The words of a map at the frame's scale that holds every point of the frame under the identity pose, MATCH_PAD cells more on
    each side where the 32768 rows or columns a map may have leave room."""
    Xp, Yp = sv.occupancy_frame_points(grid)
    ms = int(grid["scale"])
    words = dict(scale=ms, l_occ=85, l_free=40, l_min=-200, l_max=350)
    for pts, first, count in ((Xp, "top", "rows"), (Yp, "left", "cols")):
        g = np.floor(pts * float(ms)).astype(np.int64)
        n = int(g.max() - g.min()) + 1
        pad = min(MATCH_PAD, (32768 - n) // 2)
        words[first], words[count] = int(g.max()) + 1 + pad, n + 2 * pad
    return sv.occupancy_map_words(words)


def match_poses(grid):
    """float64 [8, 4]: the identity, whole and broken cells of translation inside the pad and past it, a small yaw, a quarter turn, and
    two poses that miss (far away, not finite)."""
    cell = 1.0 / grid["scale"]
    return np.array([(0.0, 0.0, 1.0, 0.0), (cell, -2 * cell, 1.0, 0.0), (-2.5 * cell, 0.25 * cell, 1.0, 0.0), (7 * cell, 5 * cell, 1.0, 0.0), (0.1, -0.1, np.cos(0.003), np.sin(0.003)),
                     (0.0, 0.0, 0.0, 1.0), (1e6, 0.0, 1.0, 0.0), (0.0, NAN, 1.0, 0.0)])


def match_states(name):
    """Two batches of three frames, the empty frame in the middle: (all occupied, all 0, exactly half and half) and (all free, bytes that
    play no part, a seeded mix of 0, 1, 2, 3 and 255)."""
    rows, cols = MATCH_CELLS[name]
    cap = rows * cols
    rng = np.random.default_rng(cap)
    half = np.ones(cap, np.uint8)
    half[rng.permutation(cap)[:cap // 2]] = 2
    mix = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), cap)
    first = np.stack([np.full(cap, 2, np.uint8), np.zeros(cap, np.uint8), half]).reshape(3, rows, cols)
    second = np.stack([np.ones(cap, np.uint8), rng.choice(np.array([0, 3, 255], np.uint8), cap), mix]).reshape(3, rows, cols)
    return first, second


def list_entries(state, w_free):
    """The entries of each frame's list: its state-2 cells, and its state-1 cells where w_free > 0."""
    return [int((st == 2).sum()) + (int((st == 1).sum()) if w_free else 0) for st in state]


CANDIDATE_COUNTS = (2047, 2048, 2049, 4097, 65535)
CANDIDATE_FRAME = dict(x_range=(0, 12), y_range=(-6, 6), scale=4)  # 49 x 49
CANDIDATE_MAP = dict(top=120, left=80, rows=160, cols=160, scale=4, l_occ=85, l_free=40, l_min=-200, l_max=350)
PLACEMENTS = ("last", "first", "two", "everywhere")
_GOOD, _POOR = (3.25, -1.5, np.cos(0.3), np.sin(0.3)), (2.0, 1.0, np.cos(-0.2), np.sin(-0.2))


def candidate_case(sv):
    """(state uint8 [49, 49] with three occupied cells, logodds int16 [160, 160]): -7 everywhere but +50 under the three cells at _GOOD,
    so that _GOOD scores 150 and _POOR -21."""
    state = np.zeros((49, 49), np.uint8)
    cells = [(5, 10), (25, 30), (40, 17)]
    for fr, fc in cells:
        state[fr, fc] = 2
    Xp, Yp = sv.occupancy_frame_points(CANDIDATE_FRAME)
    ok, r, c = sv.clearance_cells(CANDIDATE_MAP, np.array(_GOOD), [(Xp[fr], Yp[fc]) for fr, fc in cells])
    assert ok.all()
    logodds = np.full((160, 160), -7, np.int16)
    logodds[r, c] = 50
    return state, logodds


def candidate_poses(P, placement):
    """(poses float64 [P, 4], the index the best must have): _GOOD at the last index only, at index 0 only, at 300 and P - 2 - two
    indices no workgroup of up to 256 candidates shares, so that the lower one has to win across workgroups - or everywhere."""
    at = {"last": [P - 1], "first": [0], "two": [P - 2, 300], "everywhere": list(range(P))}[placement]
    p = np.tile(np.array(_POOR), (P, 1))
    p[at] = _GOOD
    return p, min(at)


def saturated_case(sv):
    """(frame grid, map words, state [2, 17, 241] - every cell occupied, every cell free: 4 x 1024 + 1 entries each - and poses [2, 257, 4]
    of whole-cell translations inside the pad): every cell lies inside the map under every candidate."""
    grid = MATCH_GRIDS["4097"]
    words = match_map(sv, grid)
    shifts = [(float(i), float(j), 1.0, 0.0) for i in (-2, 0, 3) for j in (-3, 0, 1)]
    poses = np.array([shifts[k % 9] for k in range(257)])
    state = np.stack([np.full((17, 241), 2, np.uint8), np.ones((17, 241), np.uint8)])
    return grid, words, state, np.stack([poses, poses[::-1]])


# ---------------------------------------------------------------------------------------------------------------- paths

PATH_DISCS = (2, 5, 33, 63)
PATH_STEPS = (1, 64, 65)
LONG_STEPS = 65535
LONG_R = 9


def lattice_discs(n, seed=0):
    """(centres float64 [n, 2], r2 int32 [n]): n of the 64 points of a lattice 0.75 m apart - three map cells at scale 4, more than a
    cell's diagonal, so that under any rotation no two discs share a cell - in a seeded order; r2 = 0 for disc 0, R^2 for the last."""
    rng = np.random.default_rng(900 + n + seed)
    pts = np.array([(0.75 * i - 2.625, 0.75 * j - 2.625) for i in range(8) for j in range(8)])
    centres = pts[rng.permutation(64)[:n]]
    r2 = rng.choice(np.array([0, 1, 49, 80, 81], np.int32), n)
    r2[0], r2[-1] = 0, LONG_R * LONG_R
    return np.ascontiguousarray(centres), r2


@functools.lru_cache(maxsize=None)
def long_paths(sv, n_discs, words_key):
    """-> (words, d2 uint16 [160, 160], paths float64 [3, 65535, 4], centres, r2): a seeded block of 97 poses around the map's middle,
    tiled - no footprint leaves the 6.3 m around the middle - and two poses of their own 17 m away from it on either side.  Path 0 ends on
    the first of them, path 1 starts on the second, path 2 is the block alone.  The field is far everywhere but in two cells: the
    last disc's at path 0's last step holds r2 of that disc (d2 == r2, the boundary), disc 0's at path 1's step 0 holds 0."""
    words = dict(words_key)
    ms = float(words["scale"])
    cx, cy = (words["top"] - words["rows"] / 2) / ms, (words["left"] - words["cols"] / 2) / ms
    rng = np.random.default_rng(4242 + n_discs)
    yaw = rng.uniform(-3.1, 3.1, 97)
    block = sv.occupancy_pose(cx + rng.uniform(-2, 2, 97), cy + rng.uniform(-2, 2, 97), yaw)
    tiled = np.tile(block, (LONG_STEPS // 97 + 1, 1))[:LONG_STEPS]
    paths = np.stack([tiled, tiled, tiled])
    paths[0, -1] = sv.occupancy_pose(cx + 13.0, cy - 11.0, 0.7)
    paths[1, 0] = sv.occupancy_pose(cx - 12.0, cy + 12.5, -2.1)
    centres, r2 = lattice_discs(n_discs)
    d2 = np.full((words["rows"], words["cols"]), 65535, np.uint16)
    ok, r, c = sv.clearance_cells(words, paths[0, -1], centres)
    assert ok.all()
    d2[r[-1], c[-1]] = r2[-1]
    ok, r, c = sv.clearance_cells(words, paths[1, 0], centres)
    assert ok.all()
    d2[r[0], c[0]] = 0
    return words, d2, paths, centres, r2


@functools.lru_cache(maxsize=None)
def long_paths_definition(sv, n_discs, words_key):
    """The definition on long_paths(), a path at a time (the [65535, 64] doubles of one path are enough to hold at once)."""
    words, d2, paths, centres, r2 = long_paths(sv, n_discs, words_key)
    each = [sv.clearance_paths(d2, words, paths[k:k + 1], centres, r2, LONG_R) for k in range(len(paths))]
    return {k: np.concatenate([e[k] for e in each]) for k in each[0]}
