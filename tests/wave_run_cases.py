"""Wavefront layouts built lane by lane for the four stages that combine runs of equal keys before they issue atomics - k_top_view,
k_occupancy_evidence, k_voxel_insert (wave_run / wave_run_scan of csrc/wave_ops.h) and k_ground_hist (its own ladder, issued from the
run's head) - and the keep patterns of k_cloud_write's lanes_below.  Pure numpy on top of the definitions in stereo_vision.sv (passed in
as `sv`); nothing here is random beyond the fixed seeds.  tests/test_wave_run_edges.py asserts on the CPU that every map realises the
layout it was built from, and compares the kernels and their debug counters with the definitions on the GPU.

A layout is a sequence of integer keys, one per lane, DEAD = -1 for "this lane has no point": named PATTERNS of 64 lanes joined end to
end (GROUPS), cut to a width.  With a Q whose last row is (0, 0, 0, 1) and a coordinate row (0, 0, 1, 0) a pixel's coordinate IS its
disparity, so a map paints any cell, bin or voxel into any lane: the *_map functions turn keys into disparities, the *_keys functions
recompute the keys from the map with the definition's own arithmetic, and expected_runs() is the model of the combine - it only ever
sees recomputed keys."""
import numpy as np

NAN, INF = float("nan"), float("inf")
DEAD = -1
A, B, C, TOP = 1, 2, 3, 71  # TOP: the last of N_KEYS keys - the ground histogram's last bin, which also takes everything past it
N_KEYS = 72
WIDTHS = (64, 65, 127, 128, 129, 255, 256, 257, 321)


def _ramp():
    out, r = [], 0
    while len(out) < 64:  # run lengths 1, 2, 3, ... 10 and what is left of the wavefront: 9
        out += [(A, B, C)[r % 3]] * min(r + 1, 64 - len(out))
        r += 1
    return out


PATTERNS = {
    "one_run": [A] * 64,
    "all_distinct": list(range(4, 68)),
    "alternating": [A, B] * 32,
    "halves": [A] * 32 + [B] * 32,
    "thirty_one_thirty_three": [A] * 31 + [B] * 33,  # not on the ballot's 32-bit edge
    "ramp": _ramp(),
    "tail_at_62": [A] * 63 + [B],
    "head_at_1": [B] + [A] * 63,
    "last_two": [DEAD] * 62 + [A] * 2,
    "hole": [A] * 20 + [DEAD] + [A] * 20 + [DEAD] * 2 + [A] * 21,  # dead lanes inside what would otherwise be one run: three runs
    "holes_only": [DEAD] * 64,
    "lone_63": [DEAD] * 63 + [A],
    "lone_0": [A] + [DEAD] * 63,
    "straddle_lo": [B] * 40 + [A] * 24,  # followed by straddle_hi: lane 63 and the next wavefront's lane 0 share a key - two runs
    "straddle_hi": [A] * 24 + [B] * 40,
    "top_key": [TOP] * 40 + [A] * 24,
}
# Six patterns each: a row of 321 lanes holds five and lane 0 of the sixth.  Lanes 255 | 256 - a workgroup edge of the top view, occupancy
# and ground sweeps - lie between the fourth and the fifth: the straddle in group 0, one key over three wavefronts in group 1, the two
# lone lanes in group 3.
GROUPS = (
    ("one_run", "tail_at_62", "hole", "straddle_lo", "straddle_hi", "lone_0"),
    ("straddle_lo", "straddle_hi", "all_distinct", "one_run", "one_run", "one_run"),
    ("lone_63", "lone_0", "last_two", "head_at_1", "ramp", "holes_only"),
    ("tail_at_62", "head_at_1", "alternating", "lone_63", "lone_0", "alternating"),
    ("last_two", "halves", "thirty_one_thirty_three", "top_key", "ramp", "hole"),
    ("hole", "holes_only", "one_run", "last_two", "all_distinct", "top_key"),
    ("all_distinct", "ramp", "top_key", "halves", "tail_at_62", "head_at_1"),
    ("alternating", "thirty_one_thirty_three", "holes_only", "hole", "halves", "lone_0"),
    ("ramp", "one_run", "lone_63", "thirty_one_thirty_three", "last_two", "one_run"),
)
GROUP_LANES = 6 * 64


def layout(names, width=None):
    """int64 [width]: the named patterns joined end to end, cut to a width."""
    keys = np.array([k for name in names for k in PATTERNS[name]], np.int64)
    return keys if width is None else keys[:width]


def row_keys(width):
    """int64 [2, 9, width]: one group per image row, cut to the width; the second frame is the first reversed along the row."""
    rows = np.stack([layout(g, width) for g in GROUPS])
    return np.stack([rows, rows[:, ::-1]])


def lane_sequence(width, full, turn=0):
    """int64 [2, full * GROUP_LANES + width]: `full` whole groups and one more cut to the width, starting with group `turn`; the second frame is the
    first reversed.  What the stages whose wavefronts run over one long sequence - the points of a cloud, the visited pixels of a 1 x W
    map - get instead of rows."""
    g = [GROUPS[(turn + k) % len(GROUPS)] for k in range(full + 1)]
    seq = np.concatenate([layout(n) for n in g[:full]] + [layout(g[full], width)])
    return np.stack([seq, seq[::-1]])


def expected_runs(keys, width_of_a_row):
    """The CPU model of the combine: `keys` (any shape, taken row-major as rows of width_of_a_row lanes) split into aligned segments of
    64 lanes per row, and the maximal runs of equal keys >= 0 inside each segment, as a list of (segment, first lane, length, key) -
    segments numbered through the rows, ceil(width / 64) per row, lanes 0 .. 63 inside the segment."""
    rows = np.asarray(keys).reshape(-1, width_of_a_row)
    per_row = (width_of_a_row + 63) // 64
    runs = []
    for r, row in enumerate(rows.tolist()):
        for s in range(per_row):
            seg = row[64 * s:64 * s + 64]
            lane = 0
            while lane < len(seg):
                end = lane + 1
                while end < len(seg) and seg[end] == seg[lane]:
                    end += 1
                if seg[lane] >= 0:
                    runs.append((r * per_row + s, lane, end - lane, seg[lane]))
                lane = end
    return runs


def run_slices(keys, width_of_a_row):
    """expected_runs' runs as (start, stop) into keys.reshape(-1): what a test sums labels or looks for extremes over."""
    per_row = (width_of_a_row + 63) // 64
    return [((seg // per_row) * width_of_a_row + (seg % per_row) * 64 + lane, (seg // per_row) * width_of_a_row + (seg % per_row) * 64 + lane + n)
            for seg, lane, n, _ in expected_runs(keys, width_of_a_row)]


def _cycle(where, values, dtype=np.float32):
    """The values handed out in turn to the positions where `where` holds, in row-major order."""
    out = np.zeros(where.shape, dtype)
    out[where] = np.resize(np.array(values, dtype), int(where.sum()))
    return out


# ---------------------------------------------------------------------------------------------------------------- top view

# X = d, Y = 0.5, Z = 0: with the grid below the cell row is 80 - trunc(X), the cell column 2 - trunc(0.5) = 2
TV_Q = np.array([[0, 0, 1, 0], [0, 0, 0, 0.5], [0, 0, 0, 0], [0, 0, 0, 1.0]])
TV_GRID = dict(x_range=(0, 80), y_range=(-2, 2), z_range=(-1, 1), scale=1)  # 81 x 5 cells
TV_COLS, TV_COL = 5, 2
# Y = x / 32 - 5.25: the cell column follows the pixel column, 6 - trunc(Y) on the 81 x 13 grid below
TV_Q_COLUMNS = np.array([[0, 0, 1, 0], [1 / 32, 0, 0, -5.25], [0, 0, 0, 0], [0, 0, 0, 1.0]])
TV_GRID_COLUMNS = dict(TV_GRID, y_range=(-6, 6))


def top_view_map(keys, disparity="d1"):
    """float32 disparities that put key k in cell row k.  "d1": d = 80.5 - k, X = d; the dead lanes hold NaN, -1, 0, 80.5 (out of range)
    and +inf in turn.  "dmap": d = (80 - k) / 4, so that the driver's byte 4 d = 80 - k is X - an integer, on a cell's edge; the dead
    lanes hold NaN, -1, 0, 20.25 (byte 81, out of range) and 1000 (byte 255)."""
    k = np.asarray(keys)
    if disparity == "d1":
        return np.where(k >= 0, (80.5 - k).astype(np.float32), _cycle(k < 0, [NAN, -1.0, 0.0, 80.5, INF]))
    return np.where(k >= 0, ((80 - k) / 4.0).astype(np.float32), _cycle(k < 0, [NAN, -1.0, 0.0, 20.25, 1000.0]))


def top_view_points(keys):
    """float64 [..., 3]: the point (80.5 - k, 0.5, 0) per lane; a dead lane holds a NaN point, a point past x1 and a point above z1 in turn."""
    k = np.asarray(keys)
    pts = np.stack([80.5 - k, np.full(k.shape, 0.5), np.zeros(k.shape)], -1).astype(np.float64)
    dead = np.resize(np.array([(NAN, 0.5, 0.0), (80.5, 0.5, 0.0), (40.5, 0.5, 7.0)]), (int((k < 0).sum()), 3))
    pts[k < 0] = dead
    return pts


def disparity_points(sv, d, Q, disparity="d1", labels=None):
    """float64 [..., H, W, 3]: the point of every pixel of the maps d as the stage's front end computes it (box_quantise and reproject()'s
    arithmetic, sv._box_points), NaN where the pixel is no candidate - and, with labels, where its label is neither 1 nor 2."""
    d = np.asarray(d, np.float32)
    flat = d.reshape((-1,) + d.shape[-2:])
    out = []
    for b in range(len(flat)):
        _, valid, dd = sv.box_quantise(flat[b], disparity)
        P = sv._box_points(dd, Q, None, None)
        P[~valid] = NAN
        out.append(P)
    out = np.stack(out).reshape(d.shape + (3,))
    if labels is not None:
        lab = np.asarray(labels)
        out[~((lab == 1) | (lab == 2))] = NAN
    return out


def top_view_keys(sv, points, x_range, y_range, z_range, scale):
    """int64, the shape of points[..., 0]: the flat cell row * cols + col of points_2_top_view for a point strictly inside the three
    ranges, DEAD for any other."""
    rows, cols = sv.top_view_grid(x_range, y_range, z_range, scale, "count")
    s = float(int(scale))
    p = np.asarray(points, np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(invalid="ignore"):
        ok = (x > x_range[0]) & (x < x_range[1]) & (y > y_range[0]) & (y < y_range[1]) & (z > z_range[0]) & (z < z_range[1])
    X, Y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
    row = (np.trunc(float(x_range[1]) * s) - np.trunc(X * s)).astype(np.int64)
    col = (np.trunc(float(y_range[1]) * s) - np.trunc(Y * s)).astype(np.int64)
    return np.where(ok, row * cols + col, DEAD)


def column_cells(keys):
    """The cells a map under TV_Q_COLUMNS is meant to give, in integers: row k, column 6 - trunc((x - 168) / 32) toward zero."""
    k = np.asarray(keys)
    t = np.arange(k.shape[-1], dtype=np.int64) - 168
    col = 6 - np.where(t >= 0, t // 32, -((-t) // 32))
    return np.where(k >= 0, k * 13 + col, DEAD)


# ---------------------------------------------------------------------------------------------------------------- occupancy

# (a) the cell from d as in the top view, Z = 0.875 - x / 512: with z0 = -1 and z_scale = 512 the height step is 960 - x, falling along
# the row - a run's minimum sits at its tail, its maximum at its head
OCC_Q_SLOPE = np.array([[0, 0, 1, 0], [0, 0, 0, 0.5], [-1 / 512, 0, 0, 0.875], [0, 0, 0, 1.0]])
# (b) X = 79.5 - x / 16: the cell row is 80 - (1272 - x) // 16 - blocks of 16 columns from column 9 on, so that blocks straddle lanes
# 63 | 64 and 255 | 256 -, Z = d / 512 - 1: the height step of an integer d is d
OCC_Q_BLOCKS = np.array([[-1 / 16, 0, 0, 79.5], [0, 0, 0, 0.5], [0, 0, 1 / 512, -1.0], [0, 0, 0, 1.0]])
OCC_GRID = dict(TV_GRID, z_scale=512)
OCC_LABELS = ("ground", "obstacle", "mix")


def occupancy_case(keys, labels):
    """(d float32, labels uint8) for family (a): d = 80.5 - k on the live lanes, labelled all ground, all obstacle or a seeded mix.  The
    dead lanes hold, in turn, label 0 and label 3 over the disparity of key A - no evidence under a good disparity, between lanes of the
    same cell - and NaN and -1 under labels 1 and 2."""
    k = np.asarray(keys)
    rng = np.random.default_rng(k.size)
    live = {"ground": np.ones(k.shape, np.uint8), "obstacle": np.full(k.shape, 2, np.uint8), "mix": rng.integers(1, 3, k.shape).astype(np.uint8)}[labels]
    d = np.where(k >= 0, (80.5 - k).astype(np.float32), _cycle(k < 0, [80.5 - A, 80.5 - A, NAN, -1.0]))
    lab = np.where(k >= 0, live, _cycle(k < 0, [0, 3, 1, 2], np.uint8))
    return d, lab


def occupancy_blocks(width, seed=0):
    """(d float32 [2, 9, width], labels uint8 [2, 9, width]) for family (b): every row a seeded permutation of the heights 1 .. width, the
    labels a seeded draw of 1 and 2 with 0 and 3 on about a tenth of the lanes; the second frame is the first reversed."""
    rng = np.random.default_rng(9000 + width + seed)
    d = np.stack([rng.permutation(width) + 1 for _ in range(9)]).astype(np.float32)
    lab = rng.choice(np.array([0, 1, 2, 3], np.uint8), (9, width), p=[0.05, 0.45, 0.45, 0.05])
    return np.stack([d, d[:, ::-1]]), np.stack([lab, lab[:, ::-1]])


def block_cells(d, labels):
    """The cells family (b) is meant to give, in integers: row 80 - (1272 - x) // 16, column 2, where the label is 1 or 2."""
    lab = np.asarray(labels)
    x = np.broadcast_to(np.arange(lab.shape[-1], dtype=np.int64), lab.shape)
    return np.where(((lab == 1) | (lab == 2)) & (np.asarray(d) > 0), (80 - (1272 - x) // 16) * TV_COLS + TV_COL, DEAD)


def occupancy_atomics(keys, labels, width):
    """(combined, plain): per run two atomics for the heights and one per kind of evidence the run holds; three per kept pixel."""
    k, lab = np.asarray(keys).reshape(-1), np.asarray(labels).reshape(-1)
    combined = sum(2 + int((lab[a:b] == 1).any()) + int((lab[a:b] == 2).any()) for a, b in run_slices(k, width))
    return combined, 3 * int((k >= 0).sum())


# ---------------------------------------------------------------------------------------------------------------- voxels

# P = (d, d, d): with lo = 0 and size 1 the cell is trunc(d) on all three axes, the offset inside it (d - trunc(d)) * 65536
VOXEL_Q = np.array([[0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
VOXEL_GRID = dict(size=1.0, lo=(0.0, 0.0, 0.0), hi=(float(N_KEYS),) * 3)
VOXEL_CAPACITY = 128  # >= N_KEYS voxels: no frame overflows
VOXEL_STRADDLE_W = 4096 + 70
FULL_OFFSET = np.float32(1.0 - 2.0 ** -17)  # d = c + FULL_OFFSET: the offset 65535 on all three axes (c <= 63 leaves float32 the bits)


def voxel_map(keys, frac=0.5):
    """float32: d = k + frac; the dead lanes hold NaN, -1, 0 and 72.5 (past hi) in turn."""
    k = np.asarray(keys)
    return np.where(k >= 0, k.astype(np.float32) + np.float32(frac), _cycle(k < 0, [NAN, -1.0, 0.0, N_KEYS + 0.5]))


def voxel_straddle_keys():
    """int64 [2, 1, 4166]: every group end to end, again and again, with key A over visited pixels 1010 .. 1039 - across 1023 | 1024, a tile
    edge - and 4080 .. 4109 - across 4095 | 4096, the edge of a workgroup of CLOUD_WAVES = 4 tiles; the second frame is the first reversed."""
    every = np.concatenate([layout(g) for g in GROUPS])
    seq = np.resize(every, VOXEL_STRADDLE_W)
    for at in (1010, 4080):  # thirty lanes of A between ten of B on either side
        seq[at - 10:at + 40] = B
        seq[at:at + 30] = A
    return np.stack([seq, seq[::-1]])[:, None, :]


def voxel_keys(sv, d, Q, size, lo, hi, step=1):
    """int64 [n_visited] for one map [H, W]: the packed cell c_x | c_y << 20 | c_z << 40 of voxel_cloud per visited pixel, in the order
    they are visited, DEAD where the pixel is not kept."""
    lo_, hi_, size_, cells = sv.voxel_grid(size, lo, hi, step)
    d = np.asarray(d, np.float32)
    H, W = d.shape
    P, _, index = sv.compact_cloud(d, Q, lo=lo_, hi=hi_, step=step, dtype="f64")
    c = np.minimum(((P - lo_) / np.float64(size_)).astype(np.int64), cells - 1)
    visited = (np.arange(0, H, step)[:, None] * W + np.arange(0, W, step)[None]).reshape(-1)
    keys = np.full(visited.size, DEAD, np.int64)
    keys[np.searchsorted(visited, index)] = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
    return keys


def voxel_key_of(k):
    """The packed key of cell (k, k, k), DEAD for a dead lane."""
    k = np.asarray(k, np.int64)
    return np.where(k >= 0, k | (k << 20) | (k << 40), DEAD)


# ---------------------------------------------------------------------------------------------------------------- ground

GROUND_BINS = N_KEYS


def ground_map(keys):
    """float32: d = k / 4, whose bin is k exactly; the dead lanes hold NaN, -1, 0 and -inf in turn.  The lanes of the last bin hold
    TOP / 4, +inf, 1e6 and 17.9 (4 d rounds to 72, past the last bin) in turn: all of them belong to its run."""
    k = np.asarray(keys)
    d = np.where(k >= 0, (k / 4.0).astype(np.float32), _cycle(k < 0, [NAN, -1.0, 0.0, -INF]))
    return np.where(k == TOP, _cycle(k == TOP, [TOP / 4.0, INF, 1e6, 17.9]), d)


def ground_keys(sv, d, n_bins=GROUND_BINS):
    """int64, the shape of d: ground_quantise's bin of a valid pixel, DEAD for any other."""
    q, valid = sv.ground_quantise(d, n_bins)
    return np.where(valid, q.astype(np.int64), DEAD)


# ---------------------------------------------------------------------------------------------------------------- compact cloud

def keep_patterns():
    """name -> bool [64, 4]: which of its quad's four visited pixels each lane of a wavefront keeps."""
    out = {name: np.zeros((64, 4), bool) for name in ("lane_0", "lane_63", "lanes_31_32", "pixels_0_2", "all")}
    out["lane_0"][0] = True
    out["lane_63"][63] = True
    out["lanes_31_32"][31:33] = True
    out["pixels_0_2"][:, [0, 2]] = True
    out["all"][:] = True
    return out


def keep_map(keep):
    """float32 [2, 1, 256]: a disparity of its own, 1 + v / 8, for every kept visited pixel v and -1 for the others; the second frame is
    the first reversed (with the disparities of the first, so that every row names its pixel)."""
    k = np.asarray(keep).reshape(-1)
    d = np.where(k, 1.0 + np.arange(k.size) / 8.0, -1.0).astype(np.float32)
    r = np.where(k[::-1], 1.0 + np.arange(k.size) / 8.0, -1.0).astype(np.float32)
    return np.stack([d, r])[:, None, :]
