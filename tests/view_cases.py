"""Maps, poses and rays for tests/test_view.py, painted cell by cell, and an independent model of the expected view: a per-ray loop in plain
Python with a set of visited cells, written from the prose of include/stereo_vision_hip.h (P) - it calls nothing of stereo_vision.sv.
Every case names the one mistake it is built to catch, and its `expect` checks on the CPU - against the definition's result - that the
case realises the layout it names, before a GPU sees it."""
import math

import numpy as np

FULL, HIT, EDGE, CORNER, UNKNOWN, INVALID = range(6)
OCCUPIED, FREE = 85, -40  # the thresholds of every painted map


# ---------------------------------------------------------------------------------------------------------------- the model

def model_states(logodds, last_seen, occupied, free):
    rows, cols = logodds.shape
    return [[(2 if logodds[r, c] >= occupied else 1 if logodds[r, c] <= free else 0) if last_seen[r, c] >= 0 else 0 for c in range(cols)] for r in range(rows)]


def model_view(logodds, last_seen, words, poses, ends, reach, occupied, free, max_unknown=0):
    """The result dict of the prose, cell by cell: Python floats (IEEE doubles, every operation rounded on its own) and Python integers."""
    rows, cols, top, left, ms = words["rows"], words["cols"], words["top"], words["left"], float(words["scale"])
    S = model_states(logodds, last_seen, occupied, free)
    G, P, n_rays = len(poses), len(poses[0]) if len(poses) else 0, len(ends)
    counts = np.zeros((G, P, 3), np.int32)
    end_cells = np.full((G, P, n_rays, 2), -1, np.int16)
    status = np.full((G, P, n_rays), INVALID, np.uint8)
    best, best_score = np.zeros(G, np.int32), np.zeros(G, np.int32)

    def cell_of(X, Y):  # None where the point is not finite
        a, b = X * ms, Y * ms
        if not (math.isfinite(a) and math.isfinite(b)):
            return None
        return top - 1 - math.floor(a), left - 1 - math.floor(b)

    def inside(r, c):
        return 0 <= r < rows and 0 <= c < cols

    def blocked(r, c):
        return not inside(r, c) or S[r][c] == 2

    for g in range(G):
        scores = []
        for p in range(P):
            tx, ty, c, s = (float(v) for v in poses[g][p])
            origin = cell_of(tx, ty) if all(math.isfinite(v) for v in (tx, ty, c, s)) else None
            if origin is None or not inside(*origin):
                scores.append(-1)
                continue
            r0, c0 = origin
            seen = set()
            for j in range(n_rays):
                ex, ey = float(ends[j][0]), float(ends[j][1])
                end = cell_of((c * ex - s * ey) + tx, (s * ex + c * ey) + ty)
                if end is None or abs(end[0] - r0) > reach or abs(end[1] - c0) > reach:
                    continue
                dr, dc = end[0] - r0, end[1] - c0
                n = max(abs(dr), abs(dc))
                state, last, unknown = FULL, (r0, c0), 0
                seen.add((r0, c0))
                for k in range(1, n + 1):
                    r, cc = r0 + (2 * k * dr + n) // (2 * n), c0 + (2 * k * dc + n) // (2 * n)
                    if not inside(r, cc):
                        state = EDGE
                        break
                    if r != last[0] and cc != last[1] and blocked(last[0], cc) and blocked(r, last[1]):
                        state = CORNER
                        break
                    seen.add((r, cc))
                    last = (r, cc)
                    if S[r][cc] == 2:
                        state = HIT
                        break
                    if S[r][cc] == 0:
                        unknown += 1
                        if max_unknown > 0 and unknown == max_unknown:
                            state = UNKNOWN
                            break
                status[g, p, j], end_cells[g, p, j] = state, last
            for r, cc in seen:
                counts[g, p, S[r][cc]] += 1
            scores.append(int(counts[g, p, 0]))
        best_score[g] = max(scores)
        best[g] = scores.index(max(scores))
    return {"counts": counts, "end_cells": end_cells, "status": status, "best": best, "best_score": best_score}


# ---------------------------------------------------------------------------------------------------------------- painting

def paint(text):
    """Rows of '.', '#', '?' and ' ' - free, occupied, seen but undecided, never seen - -> (logodds int16, last_seen int32)."""
    kind = np.array([[".#? ".index(ch) for ch in row] for row in text])
    logodds = np.choose(kind, [FREE, OCCUPIED, FREE + 1, OCCUPIED + 500]).astype(np.int16)  # a never-seen cell's log-odds do not count
    return logodds, np.where(kind == 3, -1, 7).astype(np.int32)


def words_of(rows, cols, scale=1, top=None, left=None):
    """The nine words of a map of rows x cols cells whose cell (0, 0) has gx = top - 1, gy = left - 1."""
    return dict(top=rows if top is None else top, left=cols if left is None else left, rows=rows, cols=cols, scale=scale, l_occ=85, l_free=40, l_min=-200, l_max=350)


def pose_in(words, r, c, yaw=0.0, fx=0.5, fy=0.5):
    """(tx, ty, cos, sin) of a vehicle that stands in cell (r, c), the fractions (fx, fy) into it along gx and gy."""
    return [(words["top"] - 1 - r + fx) / words["scale"], (words["left"] - 1 - c + fy) / words["scale"], math.cos(yaw), math.sin(yaw)]


def ends_to(words, offsets):
    """Ray ends in vehicle axes that land - from a cell's centre, at yaw 0 - in the cells (dr, dc) away: rows and columns count against x and y."""
    return np.array([[-dr / words["scale"], -dc / words["scale"]] for dr, dc in offsets], np.float64)


def fan(fov, n_rays, range_m, scale):
    """view_rays' prose, on its own: (ends, reach)."""
    a = [(j + 0.5) / n_rays * fov - fov / 2 for j in range(n_rays)]
    return np.array([[range_m * math.cos(v), range_m * math.sin(v)] for v in a], np.float64), int(math.ceil(range_m * scale)) + 1


def case(name, cells, words, poses, ends, reach, max_unknown=0, occupied=OCCUPIED, free=FREE, expect=None):
    logodds, last_seen = cells
    poses = np.asarray(poses, np.float64)
    poses = poses[None, None] if poses.ndim == 1 else poses[:, None] if poses.ndim == 2 else poses
    return dict(name=name, logodds=logodds, last_seen=last_seen, words=words, poses=poses, ends=np.asarray(ends, np.float64), reach=reach, max_unknown=max_unknown,
                occupied=occupied, free=free, expect=expect)


def args_of(c):
    return (c["logodds"], c["last_seen"], c["words"], c["poses"], c["ends"], c["reach"], c["occupied"], c["free"], c["max_unknown"])


# ---------------------------------------------------------------------------------------------------------------- the hand case

# yaw 0 looks along +x, which is up the rows; the vehicle stands in the middle of cell (3, 4)
HAND_MAP = [
    "....#....",
    "..?......",
    "..#......",
    "....... .",
    "...#.....",
    "....#....",
    ".........",
]
HAND_OFFSETS = [(-3, 0), (0, 4), (0, -4), (3, 0), (-3, -3), (3, -3), (-3, 4), (0, 0)]
# up: (2,4), (1,4), then the wall at (0,4) - seen, and it stops the ray.  right: (3,5), (3,6), the never-seen (3,7) - seen through -, (3,8).
# left: to (3,0).  down: (4,4), then the wall (5,4).  up-left: (2,3), then the undecided (1,2) - of the two cells beside that step, (2,2)
# is occupied and (1,3) free: one open side lets the ray pass -, then (0,1).  down-left: (4,3) is occupied: seen, a hit.  up-right, 3
# rows and 4 columns: the steps are (3 + floor((-6 k + 4) / 8), 4 + k) = (2,5), (2,6), (1,7), (0,8).  The last ray ends in the origin's cell.
HAND_STATUS = [HIT, FULL, FULL, HIT, FULL, HIT, FULL, FULL]
HAND_ENDS = [[0, 4], [3, 8], [3, 0], [5, 4], [0, 1], [4, 3], [0, 8], [3, 4]]
# distinct cells: the origin once; up 3 (one occupied); right 4 (one unknown); left 4; down 2 (one occupied); up-left 3 (one unknown);
# down-left 1 (occupied); up-right 4
HAND_COUNTS = [2, 17, 3]


def hand_case():
    words = words_of(7, 9)
    return case("hand", paint(HAND_MAP), words, pose_in(words, 3, 4), ends_to(words, HAND_OFFSETS), 4)


# ---------------------------------------------------------------------------------------------------------------- the cases

def _status(want, g=0, p=0):
    return lambda res: res["status"][g, p].tolist() == list(want)


def random_map(rng, rows, cols, p_occ=0.15, p_unknown=0.3):
    u = rng.random((rows, cols))
    kind = np.where(u < p_occ, 1, np.where(u < p_occ + p_unknown, rng.integers(2, 4, (rows, cols)), 0))
    logodds = np.choose(kind, [FREE, OCCUPIED, FREE + 1, OCCUPIED + 500]).astype(np.int16) + rng.integers(-3, 4, (rows, cols)).astype(np.int16) * (kind == 0)
    logodds = np.where(kind == 0, np.minimum(logodds, FREE), logodds).astype(np.int16)
    return logodds, np.where(kind == 3, -1, rng.integers(0, 9, (rows, cols))).astype(np.int32)


def device_cases():
    out = []
    free21 = paint(["." * 21] * 21)
    w21 = words_of(21, 21)
    # all eight octants, the axes, the diagonals, the origin's own cell, |dr| = reach exactly, and one beyond it on either axis and on both
    offsets = [(-7, -3), (-7, 3), (7, -3), (7, 3), (-3, -7), (-3, 7), (3, -7), (3, 7), (-7, 0), (7, 0), (0, -7), (0, 7), (-7, -7), (-7, 7), (7, -7), (7, 7), (0, 0),
               (8, 0), (0, -8), (8, 8), (-8, 7), (1, 0), (0, -1), (1, 1)]
    valid = [FULL] * 17 + [INVALID] * 4 + [FULL] * 3
    out.append(case("directions", free21, w21, pose_in(w21, 10, 10), ends_to(w21, offsets), 7,
                    expect=lambda res, valid=valid, offsets=offsets: res["status"][0, 0].tolist() == valid and res["end_cells"][0, 0, :17].tolist() == [[10 + a, 10 + b] for a, b in offsets[:17]]
                    and res["end_cells"][0, 0, 17:21].tolist() == [[-1, -1]] * 4))
    # 1024 rays within a window of 7 x 7 cells: every cell is crossed by dozens of rays and counts once; two candidates with the same rays
    rng = np.random.default_rng(3)
    w9 = words_of(9, 9)
    ends, reach = fan(2 * math.pi, 1024, 2.0, 1)
    cells9 = paint(["....?....", ".........", "..?...?..", ".........", "?.......?", "....?....", ".........", ". .......", "........."])
    out.append(case("dedup-1024", cells9, w9, [[pose_in(w9, 4, 4)], [pose_in(w9, 4, 4)]], ends, reach,
                    # the ends lie 2 m away: within the 5 x 5 cells around the origin, and the 13 cells of the disc of 2 cells are all crossed
                    expect=lambda res, reach=reach: reach == 3 and 13 <= res["counts"][0, 0].sum() <= 25 and (res["status"] == FULL).all()
                    and np.array_equal(res["counts"][0], res["counts"][1])))
    # the ray strides of a workgroup of 256 lanes and the wavefronts of 64
    cells40, w40 = random_map(rng, 40, 40), words_of(40, 40, scale=2, top=7, left=-3)
    for n_rays in (1, 63, 64, 65, 255, 256, 257, 1024):
        ends, reach = fan(1.7, n_rays, 6.3, 2)
        poses = [[pose_in(w40, 20, 20, 0.3, 0.25, 0.75), pose_in(w40, 5, 33, 2.0), pose_in(w40, 38, 1, -1.1, 0.0, 0.0)]]
        out.append(case("rays-%d" % n_rays, cells40, w40, poses, ends, reach, expect=lambda res, n=n_rays: res["status"].shape == (1, 3, n) and (res["status"] != INVALID).all()))
    # the largest window: 509 cells a side, a ray to each of its corners and along each axis - bits 0 and 508 of a row, rows 0 and 508
    big = np.full((512, 512), FREE, np.int16), np.zeros((512, 512), np.int32)
    big[0][3, 255], big[0][255, 509] = FREE + 1, FREE + 1
    w512 = words_of(512, 512)
    offsets = [(-254, -254), (-254, 254), (254, -254), (254, 254), (0, -254), (0, 254), (-254, 0), (254, 0), (-254, 1), (255, 0), (0, -255)]
    out.append(case("window-254", big, w512, pose_in(w512, 255, 255), ends_to(w512, offsets), 254,
                    expect=lambda res: res["status"][0, 0].tolist() == [FULL] * 9 + [INVALID] * 2 and res["end_cells"][0, 0, :4].tolist() == [[1, 1], [1, 509], [509, 1], [509, 509]]
                    # the origin, 8 rays of 254 cells of their own, and the ray to (-254, 1): column 255 + floor((2 k + 254) / 508), which leaves the
                    # column of the ray beside it at k = 127 - 128 cells of its own; two of all those cells are undecided
                    and res["counts"][0, 0].sum() == 1 + 8 * 254 + 128 and res["counts"][0, 0].tolist() == [2, 2159, 0]))
    # rows of the bitmap of 31, 33, 63 and 65 bits (2 reach + 1 is odd: rows of 32 and 64 bits do not exist): 1, 2, 2 and 3 words
    w70 = words_of(70, 70)
    cells70 = random_map(rng, 70, 70, 0.02, 0.4)
    for reach in (15, 16, 31, 32):
        offsets = [(-reach, -reach), (reach, reach), (0, -reach), (0, reach), (reach, -reach), (-reach, reach), (-reach, 0), (reach, 0), (3, reach), (-reach, -2)]
        out.append(case("row-bits-%d" % (2 * reach + 1), cells70, w70, pose_in(w70, 35, 35), np.concatenate([ends_to(w70, offsets), fan(2 * math.pi, 90, reach - 1.0, 1)[0]]), reach,
                        expect=lambda res: (res["status"] != INVALID).all()))
    # an origin in each corner of the map; maps of one cell, one row and one column
    fan_ends, fan_reach = fan(2 * math.pi, 64, 5.0, 1)
    cells12, w12 = random_map(rng, 12, 17, 0.05, 0.3), words_of(12, 17)
    out.append(case("map-corners", cells12, w12, [[pose_in(w12, 0, 0), pose_in(w12, 0, 16), pose_in(w12, 11, 0), pose_in(w12, 11, 16)]], fan_ends, fan_reach,
                    expect=lambda res: all((res["status"][0, p] == EDGE).sum() >= 32 for p in range(4))))
    w1 = words_of(1, 1)
    out.append(case("map-1x1", paint(["?"]), w1, pose_in(w1, 0, 0), fan_ends, fan_reach, expect=lambda res: res["counts"][0, 0].tolist() == [1, 0, 0] and (res["status"] == EDGE).all()
                    and (res["end_cells"] == 0).all()))
    for shape in ((1, 40), (40, 1)):
        w = words_of(*shape)
        cells = random_map(rng, shape[0], shape[1], 0.0, 0.3)
        at = (0, 20) if shape[0] == 1 else (20, 0)
        out.append(case("map-%dx%d" % shape, cells, w, pose_in(w, *at), fan_ends, fan_reach, expect=lambda res: res["counts"][0, 0].sum() == 11 and (res["status"] == EDGE).sum() >= 60))
    # the corner guard.  The vehicle stands in (3, 1), the rays go up and to the right.
    w5 = words_of(5, 5)
    both = paint([".....", ".....", ".#...", "..#..", "....."])   # the step (3,1) -> (2,2) has (3,2) and (2,1) beside it
    one = paint([".....", ".....", ".....", "..#..", "....."])
    other = paint([".....", ".....", ".#...", ".....", "....."])
    diag = ends_to(w5, [(-2, 2)])
    out.append(case("corner-both", both, w5, pose_in(w5, 3, 1), diag, 3, expect=lambda res: res["status"][0, 0, 0] == CORNER and res["end_cells"][0, 0, 0].tolist() == [3, 1]
                    and res["counts"][0, 0].tolist() == [0, 1, 0]))
    for name, cells in (("corner-one-a", one), ("corner-one-b", other)):
        out.append(case(name, cells, w5, pose_in(w5, 3, 1), diag, 3, expect=lambda res: res["status"][0, 0, 0] == FULL and res["end_cells"][0, 0, 0].tolist() == [1, 3]
                        and res["counts"][0, 0].tolist() == [0, 3, 0]))
    # a diagonal step out of the map: the cell itself is outside, which is tested first - the edge, whatever stands beside the step
    out.append(case("corner-outside", paint([".#...", ".....", ".....", ".....", "....."]), w5, pose_in(w5, 0, 0), ends_to(w5, [(-2, 2), (2, -2)]), 3,
                    expect=lambda res: res["status"][0, 0].tolist() == [EDGE, EDGE] and res["end_cells"][0, 0].tolist() == [[0, 0], [0, 0]]))
    # a wall one cell thick along a diagonal: no ray of a dense fan from below it sees a cell above it; a ray along an axis hits it
    w11 = words_of(11, 11)
    wall = ["." * 11 for _ in range(11)]
    wall = [row[:10 - r] + "#" + row[11 - r:] for r, row in enumerate(wall)]  # (r, 10 - r)
    ends, reach = fan(2 * math.pi, 720, 7.0, 1)
    ends = np.concatenate([ends, ends_to(w11, [(-4, 0), (0, -4)])])

    def behind_the_wall(res):
        e = res["end_cells"][0, 0].astype(int)
        return (e[:, 0] + e[:, 1] >= 10).all() and (res["status"][0, 0] == CORNER).sum() > 0 and res["status"][0, 0, 720:].tolist() == [HIT, HIT] and e[720:].tolist() == [[4, 6], [8, 2]]
    out.append(case("corner-diagonal-wall", paint(wall), w11, pose_in(w11, 8, 6), ends, reach, expect=behind_the_wall))
    # max_unknown on a ray through three undecided cells, a free one, and two more
    w10 = words_of(1, 10)
    run = paint([".???.??..."])
    for m, want, end in ((0, FULL, 9), (1, UNKNOWN, 1), (2, UNKNOWN, 2), (3, UNKNOWN, 3), (4, UNKNOWN, 5), (5, UNKNOWN, 6), (6, FULL, 9), (255, FULL, 9)):
        out.append(case("max-unknown-%d" % m, run, w10, pose_in(w10, 0, 0), ends_to(w10, [(0, 9)]), 10, max_unknown=m,
                        expect=lambda res, want=want, end=end: res["status"][0, 0, 0] == want and res["end_cells"][0, 0, 0].tolist() == [0, end]))
    # an origin on an undecided cell: step 0 does not count towards max_unknown
    out.append(case("max-unknown-origin", paint(["??.?"]), words_of(1, 4), pose_in(words_of(1, 4), 0, 0), ends_to(words_of(1, 4), [(0, 3)]), 4, max_unknown=2,
                    expect=lambda res: res["status"][0, 0, 0] == UNKNOWN and res["end_cells"][0, 0, 0].tolist() == [0, 3] and res["counts"][0, 0].tolist() == [3, 1, 0]))
    # the thresholds: at occupied and one below, at free and one above, and never seen under a large log-odds
    w6 = words_of(1, 7)
    L = np.array([[FREE, FREE, FREE + 1, OCCUPIED - 1, 3000, OCCUPIED, FREE]], np.int16)
    seen = np.array([[0, 0, 0, 5, -1, 0, 0]], np.int32)
    out.append(case("thresholds", (L, seen), w6, pose_in(w6, 0, 0), ends_to(w6, [(0, 6)]), 7,
                    expect=lambda res: res["status"][0, 0, 0] == HIT and res["end_cells"][0, 0, 0].tolist() == [0, 5] and res["counts"][0, 0].tolist() == [3, 2, 1]))
    out.append(case("thresholds-shifted", (L, seen), w6, pose_in(w6, 0, 0), ends_to(w6, [(0, 6)]), 7, occupied=OCCUPIED + 1, free=FREE - 1,
                    expect=lambda res: res["status"][0, 0, 0] == FULL and res["counts"][0, 0].tolist() == [7, 0, 0]))
    out.append(case("thresholds-low", (L, seen), w6, pose_in(w6, 0, 0), ends_to(w6, [(0, 6)]), 7, occupied=OCCUPIED - 1, free=FREE + 1,
                    expect=lambda res: res["status"][0, 0, 0] == HIT and res["end_cells"][0, 0, 0].tolist() == [0, 3] and res["counts"][0, 0].tolist() == [0, 3, 1]))
    # the best: ties go to the lowest index; a group of invalid candidates; one candidate per group
    w8 = words_of(3, 8)
    tie = paint(["........", "?......?", "........"])
    nan, inf = float("nan"), float("inf")
    look = ends_to(w8, [(0, -3), (0, 3)])
    poses = [[pose_in(w8, 0, 4), pose_in(w8, 1, 3), pose_in(w8, 1, 4), pose_in(w8, 1, 3)],        # 0, 1, 1, 1 unknown cells: best 1
             [[nan, 1.0, 1.0, 0.0], [1.0, inf, 1.0, 0.0], [99.5, 1.5, 1.0, 0.0], [1.5, 1.5, nan, 0.0]],  # nothing valid: best 0, score -1
             [[nan, 1.0, 1.0, 0.0], pose_in(w8, 0, 6), pose_in(w8, 0, 0), pose_in(w8, 0, 6)]]     # an invalid one first: 0 unknown cells beat -1
    out.append(case("best", tie, w8, poses, look, 3, expect=lambda res: res["best"].tolist() == [1, 0, 1] and res["best_score"].tolist() == [1, -1, 0]
                    and (res["status"][1] == INVALID).all() and (res["end_cells"][1] == -1).all() and not res["counts"][1].any()))
    out.append(case("best-p1", tie, w8, [[pose_in(w8, 1, 3)], [[nan, 0.0, 1.0, 0.0]], [pose_in(w8, 0, 6)]], look, 3,
                    expect=lambda res: res["best"].tolist() == [0, 0, 0] and res["best_score"].tolist() == [1, -1, 0]))
    # many workgroups: 2049 groups of one candidate with two rays each
    many = np.array([pose_in(w40, int(r), int(c), float(y)) for r, c, y in zip(rng.integers(-2, 42, 2049), rng.integers(-2, 42, 2049), rng.uniform(-4, 4, 2049))])
    out.append(case("groups-2049", cells40, w40, many, [[2.0, 0.25], [-1.0, 1.5]], 6, expect=lambda res: res["best"].shape == (2049,) and 50 < (res["best_score"] < 0).sum() < 400))
    return out


def random_cases(n=30, seed=17):
    """Random maps of 1 .. 40 cells a side and random poses: origins on the edge rows and columns and outside the map, words that are NaN or
    inf, (c, s) that is no rotation, rays beyond reach."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        rows, cols = (int(v) for v in rng.integers(1, 41, 2))
        scale = int(rng.choice([1, 2, 3, 10]))
        words = words_of(rows, cols, scale, top=int(rng.integers(-50, 50)), left=int(rng.integers(-50, 50)))
        G, P = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        poses = np.zeros((G, P, 4))
        for g in range(G):
            for p in range(P):
                kind = int(rng.integers(0, 8))
                r, c = int(rng.integers(0, rows)), int(rng.integers(0, cols))
                if kind == 0:
                    r = int(rng.choice([0, rows - 1]))
                elif kind == 1:
                    c = int(rng.choice([0, cols - 1]))
                elif kind == 2:
                    r, c = int(rng.choice([-1, rows, -7])), int(rng.choice([-1, cols, c]))
                poses[g, p] = pose_in(words, r, c, float(rng.uniform(-7, 7)), float(rng.random()), float(rng.random()))
                if kind == 3:
                    poses[g, p, int(rng.integers(0, 4))] = [np.nan, np.inf, -np.inf][int(rng.integers(0, 3))]
                elif kind == 4:
                    poses[g, p, 2:] *= rng.uniform(0.3, 1.6, 2)  # no rotation: the ends scale and shear; some leave the reach
        ends, reach = fan(float(rng.uniform(0.2, 2 * math.pi)), int(rng.integers(1, 40)), float(rng.uniform(0.3, 12.0 / scale)), scale)
        out.append(case("random-%d" % k, random_map(rng, rows, cols), words, poses, ends, reach, max_unknown=int(rng.choice([0, 0, 1, 3, 255]))))
    return out
