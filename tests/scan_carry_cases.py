"""Cases built thread by thread for the stages that hand a value from one thread to the next through csrc/wave_ops.h's scans and
reductions and add a carry of their own on top: k_stixel_objects (running maximum of the segment starts, prefix sum of the kept
segments, carry_start / carry_kept from chunk to chunk, strided min / max / median), k_box_positions (block scan over 4096 bins at 16 a
thread, the column sums 256 at a time), k_ground_hist / k_ground_search / k_ground_pick (the in-place bin scan, the arg-max by key),
k_cloud_scan (the tile prefix sum) and k_voxel_write (a lane's rank from the popcount of its 16 mask bits).  Pure numpy: the
definitions of stereo_vision.sv are passed in as `sv` where a builder needs them.

Every family comes with a numpy MODEL of the kernel's carry step that takes the name of ONE mistake (`bug`): with bug=None the model
is the definition, with the mistake a case is aimed at it is not - tests/test_scan_carry_edges.py asserts both on the CPU, and compares
the kernels with the definitions on the GPU."""
import collections

import numpy as np

NAN, INF = float("nan"), float("inf")
POISON = -77
THREADS = 256  # of every workgroup modelled here


def _wave_exclusive(vals, drop_wave_base=False):
    """block_exclusive_scan over 256 values -> (exclusive prefix per thread, total); drop_wave_base: the wavefront totals before the
    thread's own wavefront are left out."""
    v = np.asarray(vals, np.int64)
    excl = np.cumsum(v) - v
    if drop_wave_base:
        excl = excl - np.repeat(excl[::64], 64)
    return excl, int(v.sum())


# ---------------------------------------------------------------------------------------------------------------- stixel objects

STIXEL_SPEC = dict(n_bins=4096, q_min=0, sim=0, max_gap=0, min_rows=1, max_layers=1)
STIXEL_WIDTHS = (64, 65, 255, 256, 257, 511, 512, 513, 769, 1025)
STIXEL_EDGES = (63, 127, 191, 255, 511, 767)  # the left cell of each edge
STIXEL_BUGS = ("start_wave_base", "start_carry_dropped", "start_carry_forgotten", "kept_wave_base", "kept_carry_dropped", "sim_ge", "sim_gt_plus_one",
               "min_cols_gt", "length_plus_one", "capacity_minus_one", "capacity_plus_one", "upper_median", "first_stride_only", "half_wave_reduce")

StixelCase = collections.namedtuple("StixelCase", "name q top bottom col_step sim_cols min_cols capacity segments q_med aimed")


def stixel_map(q, top=None, bottom=None, col_step=1):
    """(d float32 [4, W], labels uint8 [4, W]) whose first layer under STIXEL_SPEC is stixel_layer0(q, top, bottom): visited column i
    holds the disparity q[i] / 4 (0.0625 for bin 0: valid, and 4 d rounds to 0) under label 2 on the rows top[i] .. bottom[i] and label 1
    on the others; q[i] < 0 is a gap, label 1 throughout.  The columns between the visited ones hold a stixel of bin 28 nobody visits."""
    q = np.asarray(q, np.int64)
    Wv = len(q)
    top = np.zeros(Wv, np.int64) if top is None else np.asarray(top, np.int64)
    bottom = np.full(Wv, 3, np.int64) if bottom is None else np.asarray(bottom, np.int64)
    W = (Wv - 1) * col_step + 1
    d, lab = np.full((4, W), 7.0, np.float32), np.full((4, W), 2, np.uint8)
    u = np.arange(Wv) * col_step
    rows = np.arange(4)[:, None]
    d[:, u] = np.where(q > 0, q / 4.0, 0.0625).astype(np.float32)[None]
    lab[:, u] = np.where((q >= 0)[None] & (rows >= top[None]) & (rows <= bottom[None]), 2, 1)
    return d, lab


def stixel_layer0(q, top=None, bottom=None):
    """int32 [Wv, 4]: (v_bottom, v_top, q, rows) per visited column, -1 for a gap."""
    q = np.asarray(q, np.int64)
    top = np.zeros(len(q), np.int64) if top is None else np.asarray(top, np.int64)
    bottom = np.full(len(q), 3, np.int64) if bottom is None else np.asarray(bottom, np.int64)
    out = np.stack([bottom, top, q, bottom - top + 1], -1)
    out[q < 0] = -1
    return out.astype(np.int32)


def stixel_objects_model(layer0, col_step, sim_cols, min_cols, capacity, bug=None):
    """k_stixel_objects thread by thread, chunk by chunk -> (boxes, info, count) in the definition's shapes: min(count, capacity) rows,
    POISON in a row the kernel would not have written.  bug names the one mistake made (STIXEL_BUGS), None = none."""
    assert bug is None or bug in STIXEL_BUGS
    L = np.asarray(layer0, np.int64)
    Wv = len(L)
    has, q = L[:, 0] >= 0, L[:, 2]
    split_at = sim_cols + (1 if bug == "sim_gt_plus_one" else 0)
    differs = (lambda a, b: abs(a - b) >= split_at) if bug == "sim_ge" else (lambda a, b: abs(a - b) > split_at)
    rows = {}
    carry_start, carry_kept = -1, 0
    for base in range(0, Wv, THREADS):
        start, ends = np.full(THREADS, -1, np.int64), np.zeros(THREADS, bool)
        for t in range(min(THREADS, Wv - base)):
            i = base + t
            if has[i]:
                if i == 0 or not has[i - 1] or differs(q[i], q[i - 1]):
                    start[t] = i
                ends[t] = i + 1 >= Wv or not has[i + 1] or differs(q[i + 1], q[i])
        run = np.maximum.accumulate(start.reshape(4, 64), axis=1)  # wave_inclusive_max
        totals = run[:, 63]
        carry_in = -1 if bug == "start_carry_dropped" else carry_start
        kept, seg_start = np.zeros(THREADS, bool), np.zeros(THREADS, np.int64)
        for t in range(THREADS):
            w = t >> 6
            before = carry_in
            if bug != "start_wave_base":
                before = max([before] + [int(x) for x in totals[:w]])
            seg_start[t] = max(int(run[w, t & 63]), before)
            n = base + t - seg_start[t] + 1 + (1 if bug == "length_plus_one" else 0)
            kept[t] = ends[t] and (n > min_cols if bug == "min_cols_gt" else n >= min_cols)
        everything = max([-1 if bug == "start_carry_forgotten" else carry_in] + [int(x) for x in totals])
        local, total = _wave_exclusive(kept, bug == "kept_wave_base")
        queue = {}
        for t in np.nonzero(kept)[0]:
            if carry_kept + local[t] < capacity:
                queue[int(local[t])] = (int(seg_start[t]), base + int(t))
        room = capacity - carry_kept + {"capacity_minus_one": -1, "capacity_plus_one": 1}.get(bug, 0)
        for k in range(min(max(room, 0), total)):
            if k not in queue:  # the kernel would read a stale queue entry and write a row with it
                rows[carry_kept + k] = ((-1,) * 4, (-1,) * 4)
                continue
            c0, c1 = queue[k]
            o = np.arange(c1 - c0 + 1)
            if bug == "first_stride_only":
                o = o[o < 64]
            if bug == "half_wave_reduce":
                o = o[(o & 63) < 32]
            cols = L[np.clip(c0 + o, 0, Wv - 1)]
            n_cols = c1 - c0 + 1
            rank = n_cols // 2 + 1 if bug == "upper_median" else (n_cols + 1) // 2
            qs = np.sort(cols[:, 2]) if len(cols) else np.array([POISON])
            v_top = int(cols[:, 1].min()) if len(cols) else POISON
            v_bot = int(cols[:, 0].max()) if len(cols) else POISON
            q_med = int(qs[min(rank, len(qs)) - 1])
            rows[carry_kept + k] = ((c0 * col_step, v_top, (c1 - c0) * col_step + 1, v_bot - v_top + 1), (n_cols, int(qs[0]), int(qs[-1]), q_med))
        carry_start = everything
        carry_kept = total if bug == "kept_carry_dropped" else carry_kept + total
    n = max(min(carry_kept, capacity), max(rows, default=-1) + 1)
    boxes, info = np.full((n, 4), POISON, np.int32), np.full((n, 4), POISON, np.int32)
    for r, (bx, nf) in rows.items():
        boxes[r], info[r] = bx, nf
    return boxes, info, carry_kept


def _stixel_case(name, q, segments, aimed, top=None, bottom=None, col_step=1, sim_cols=2, min_cols=3, capacity=64, q_med=None):
    return StixelCase(name, np.asarray(q, np.int64), top, bottom, col_step, sim_cols, min_cols, capacity, tuple(segments), q_med, tuple(aimed))


def _edge_bugs(edge, start):
    """The mistakes a segment at this edge shows: a wavefront's or a chunk's; start: in the running maximum, else in the prefix sum."""
    chunk = edge % THREADS == THREADS - 1
    if start:
        return ("start_carry_dropped",) if chunk else ("start_wave_base",)
    return ("kept_carry_dropped",) if chunk else ("kept_wave_base",)


def stixel_edge_cases(width):
    """The cases of one width (visited columns) for every edge that lies inside it.  A decoy segment on columns 2 .. 6 comes first, so
    that a lost start or a lost row count has something wrong to fall back on.  Every width also has a segment on its last columns."""
    gaps = np.full(width, -1, np.int64)
    gaps[2:7] = 40
    q = gaps.copy()
    q[width - 4:] = 100  # min_cols columns that end with the map: no right neighbour to ask
    out = [_stixel_case("tail_%d" % width, q, [(2, 6), (width - 4, width - 1)], ("min_cols_gt",), min_cols=4)]
    for e in [e for e in STIXEL_EDGES if e + 1 < width]:
        lo, hi = e - 9, min(e + 10, width - 1)
        # a segment that ends on the left cell and one that begins on the right cell: bins 100 and 200, more than sim_cols apart
        q = gaps.copy()
        q[lo:e + 1], q[e + 1:hi + 1] = 100, 200
        segs = [(2, 6), (lo, e)] + ([(e + 1, hi)] if hi - e >= 3 else [])
        if hi - e >= 3:
            out.append(_stixel_case("split_%d_%d" % (e, width), q, segs, _edge_bugs(e, False)))
        # one segment across the edge
        q = gaps.copy()
        q[lo:hi + 1] = 100
        out.append(_stixel_case("across_%d_%d" % (e, width), q, [(2, 6), (lo, hi)], _edge_bugs(e, True)))
        # |dq| = sim_cols joins, sim_cols + 1 splits, exactly at the edge
        for dq, name in ((2, "joins"), (3, "splits")):
            q = gaps.copy()
            q[lo:e + 1], q[e + 1:hi + 1] = 100, 100 + dq
            segs = [(2, 6), (lo, hi)] if dq == 2 else [(2, 6), (lo, e)] + ([(e + 1, hi)] if hi - e >= 3 else [])
            out.append(_stixel_case("sim_%s_%d_%d" % (name, e, width), q, segs, ("sim_ge",) if dq == 2 else ("sim_gt_plus_one",)))
        # across the edge with exactly min_cols columns, and with one less
        if e + 2 < width:
            for n, name in ((4, "min_cols"), (3, "min_cols_less_one")):
                q = gaps.copy()
                q[e - 1:e - 1 + n] = 100
                segs = [(2, 6)] + ([(e - 1, e + 2)] if n == 4 else [])
                out.append(_stixel_case("%s_%d_%d" % (name, e, width), q, segs, (_edge_bugs(e, True) + ("min_cols_gt",)) if n == 4 else ("length_plus_one",), min_cols=4))
    return out


def stixel_long_cases():
    """One segment over the whole width where it takes two, three and five chunks; a segment from chunk 0 into chunk 2 with gaps
    everywhere else (chunk 1 holds no start: the carry has to survive it)."""
    out = []
    for width in (257, 513, 1025):
        out.append(_stixel_case("whole_%d" % width, np.full(width, 100), [(0, width - 1)], ("start_carry_dropped",) + (("start_carry_forgotten",) if width > 512 else ())))
    q = np.full(769, -1, np.int64)
    q[200:601] = 100
    out.append(_stixel_case("chunk_0_to_2", q, [(200, 600)], ("start_carry_dropped", "start_carry_forgotten")))
    return out


STIXEL_LENGTHS = (1, 63, 64, 65, 128, 129)
STIXEL_MULTISETS = ("equal", "two_values", "full_range", "median_at_63", "median_at_64")


def stixel_median_cases():
    """Segments of STIXEL_LENGTHS columns from column 5 of a 160-column map, any bins joined (sim_cols 4096, min_cols 1), for the strided
    min / max / median loops.  The segment's last column alone reaches row 0 and its first alone row 3, so that a lane or a stride left
    out of a reduction shows in the box whatever the bins are."""
    out = []
    for n in STIXEL_LENGTHS:
        for kind in STIXEL_MULTISETS:
            if (kind == "median_at_63" and n < 64) or (kind == "median_at_64" and n < 65):
                continue
            rank = (n + 1) // 2
            if kind == "equal":
                seg, med = np.full(n, 300), 300
            elif kind == "two_values":  # the lower median is 300 by exactly one column
                seg, med = np.array([300] * rank + [400] * (n - rank))[np.random.default_rng(n).permutation(n)], 300
            elif kind == "full_range":
                seg, med = np.array([0] + [1000] * (n - 2) + [4095] * (n > 1)), (0 if n <= 2 else 1000)
            else:  # one column holds the median value: rank - 1 columns below it, the rest above
                at = 63 if kind == "median_at_63" else 64
                rest = np.array([300] * (rank - 1) + [500] * (n - rank))[np.random.default_rng(n + at).permutation(n - 1)]
                seg, med = np.insert(rest, at, 400), 400
            q = np.full(160, -1, np.int64)
            q[5:5 + n] = seg
            top, bottom = np.full(160, 1), np.full(160, 2)
            top[5 + n - 1], bottom[5] = 0, 3
            aimed = ["min_cols_gt"] if n == 1 else ["first_stride_only" if n > 64 else "half_wave_reduce"]
            if kind in ("two_values", "median_at_63", "median_at_64") and n % 2 == 0:
                aimed.append("upper_median")
            out.append(_stixel_case("median_%s_%d" % (kind, n), q, [(5, 4 + n)], aimed, top=top, bottom=bottom, sim_cols=4096, min_cols=1, q_med=med))
    return out


def stixel_short_segments(width=513):
    """Segments of two columns end to end, their bins 50, 57, 64 in turn: 128 of them in chunk 0 - 32 per wavefront -, 128 in chunk 1 and
    column 512 on its own (one column: not kept)."""
    return ((np.arange(width) // 2) % 3) * 7 + 50


STIXEL_SHORT_TOTAL = 256
STIXEL_CAPACITIES = (0, 1, 50, 128, 129, 200, 255, 256)  # inside chunk 0, its end exactly, that plus 1, inside chunk 1, the total minus 1, the total


def stixel_capacity_cases():
    q = stixel_short_segments()
    segs = [(2 * k, 2 * k + 1) for k in range(STIXEL_SHORT_TOTAL)]
    out = []
    for cap in STIXEL_CAPACITIES:
        aimed = ["capacity_plus_one"] + (["capacity_minus_one"] if cap else []) + (["kept_wave_base"] if cap > 32 else []) + (["kept_carry_dropped"] if cap > 128 else [])
        out.append(_stixel_case("capacity_%d" % cap, q, segs[:cap], aimed if cap < STIXEL_SHORT_TOTAL else aimed[1:], min_cols=2, capacity=cap))
    one_chunk = _stixel_case("short_one_chunk", q[:256], segs[:128], ("kept_wave_base",), min_cols=2, capacity=128)
    return [one_chunk] + out


def stixel_cases():
    """name -> StixelCase, every case of the family."""
    cases = [c for w in STIXEL_WIDTHS for c in stixel_edge_cases(w)] + stixel_long_cases() + stixel_median_cases() + stixel_capacity_cases()
    e = [c for c in stixel_edge_cases(257)]
    cases += [c._replace(name=c.name + "_step3", col_step=3) for c in e]
    out = collections.OrderedDict((c.name, c) for c in cases)
    assert len(out) == len(cases)
    return out


# ---------------------------------------------------------------------------------------------------------------- box median and sums

BOX_BINS, BOX_PER = 4096, 16  # bins, and bins per thread of the scan
# X = (x - 300.5) * 0.54 / d and so on: quotients that no double holds, so the order of the additions shows
BOX_Q = np.array([[1, 0, 0, -300.5], [0, 1, 0, -0.7], [0, 0, 0, 721.3], [0, 0, 1 / 0.54, 0.0]])
BOX_MEDIANS = {"d1": (0, 1, 15, 16, 17, 1023, 1024, 4079, 4080, 4095), "dmap": (1, 15, 16, 255)}
BOX_TOP = {"d1": 4095, "dmap": 255}
BOX_KINDS = ("one", "two", "odd", "even_next_thread", "even_next_wave", "one_bin")
BOX_BUGS = ("wave_base", "thread_base", "walk_gt", "select_le", "upper_median", "total_without_wave_0", "total_without_wave_1", "total_without_wave_3", "band_lt")
BOX_MEDIAN_WIDTH = 24  # columns of a median box: the valid pixels first, invalid ones behind them
BOX_SUM_BUGS = ("chunk_carry", "last_column", "first_column", "right_to_left")

BoxCase = collections.namedtuple("BoxCase", "name disparity bins median n_valid aimed")


def box_disparity(bins, disparity):
    """float32: a disparity per bin - bin / 4, 0.0625 for bin 0 (valid under "d1" only, and 4 d rounds to 0), -1 for bin -1: not valid."""
    b = np.asarray(bins, np.int64)
    return np.where(b > 0, b / 4.0, np.where(b == 0, 0.0625, -1.0)).astype(np.float32)


def box_median_bins(m, kind, top):
    """The bins of a box's valid pixels, in a seeded order, whose lower median is m - by exactly one pixel: `below` pixels under m, as many
    at m as it takes to reach the rank, the next one in the partner bin, the rest far above.  None where the kind cannot be built: no
    partner bin above the top bin, none 1024 bins up."""
    n = {"one": 1, "two": 2, "odd": 9, "even_next_thread": 10, "even_next_wave": 10, "one_bin": 7}[kind]
    if kind == "one_bin":
        return np.full(n, m, np.int64)
    partner = {"even_next_thread": (m // BOX_PER + 1) * BOX_PER + 3, "even_next_wave": (m // 1024 + 1) * 1024}.get(kind, m + 1)
    if n > 1 and partner > top:
        return None if kind.startswith("even") else np.array([m - 1] * ((n + 1) // 2 - 1) + [m] * (n // 2 + 1), np.int64)  # the top bin: both middle pixels in it
    lowest = 0 if top > 255 else 1  # bin 0 is not valid under "dmap"
    rank = (n + 1) // 2
    below = rank - 1 if m > lowest else 0
    far_below, far_above = min(lowest + 5, m - 1), min(partner + 900, top)  # in thread 0 where m is not; wavefront 0 where m is not
    bins = [far_below] * (below // 2) + [m - 1] * (below - below // 2) + [m] * (rank - below) + [partner] * min(1, n - rank) + [far_above] * max(n - rank - 1, 0)
    return np.array(bins, np.int64)[np.random.default_rng(m + n).permutation(n)]


def box_histogram(bins):
    return np.bincount(np.asarray(bins, np.int64), minlength=BOX_BINS)


def box_median_cases():
    """Every (disparity form, median bin, kind) that can be built; aimed = the mistakes of BOX_BUGS that box_median_model makes visible
    on the case (the CPU test asserts that there is one, and which kinds must show which)."""
    out = []
    for disparity, medians in BOX_MEDIANS.items():
        for m in medians:
            for kind in BOX_KINDS:
                bins = box_median_bins(m, kind, BOX_TOP[disparity])
                if bins is None:
                    continue
                hist = box_histogram(bins)
                want = box_median_model(hist)
                aimed = tuple(bug for bug in BOX_BUGS[:-1] if box_median_model(hist, bug) != want)
                out.append(BoxCase("%s_%d_%s" % (disparity, m, kind), disparity, bins, m, len(bins), aimed))
    return out


def box_band_bins(m):
    """13 valid pixels with lower median m: 2 at m - 2, 2 at m - 1, 3 at m, 3 at m + 1, 2 at m + 2 and one far above: the band 0 selects
    3, the band 1 selects 8, the band 2 selects 12."""
    return np.array([m - 2] * 2 + [m - 1] * 2 + [m] * 3 + [m + 1] * 3 + [m + 2] * 2 + [m + 40], np.int64)[np.random.default_rng(m).permutation(13)]


BOX_BAND_MEDIANS = {"d1": (15, 1023), "dmap": (15,)}
BOX_BAND_SELECTED = {0: 3, 1: 8, 2: 12}


def box_median_map(bins, disparity, width=BOX_MEDIAN_WIDTH):
    """(d float32 [2, width + 1], box): one row of the bins' disparities, invalid pixels behind them, and the box that holds that row."""
    row = np.full(width + 1, -1, np.int64)
    row[:len(bins)] = bins
    d = np.stack([box_disparity(row, disparity), box_disparity(np.full(width + 1, 77), disparity)])
    return d, (0, 0, width, 1)


def box_median_model(hist, bug=None):
    """The median step of k_box_positions on a histogram of 4096 bins -> (n_valid, the sorted list of the bins some thread would store
    as the median: one thread, one bin when all is well; [] leaves -1)."""
    assert bug is None or bug in BOX_BUGS
    hist = np.asarray(hist, np.int64)
    own = hist.reshape(THREADS, BOX_PER).sum(1)
    excl, n_valid = _wave_exclusive(own, bug == "wave_base")
    incl = excl + own
    if bug and bug.startswith("total_without_wave_"):
        n_valid -= int(own[64 * int(bug[-1]):64 * int(bug[-1]) + 64].sum())
    rank = n_valid // 2 + 1 if bug == "upper_median" else (n_valid + 1) // 2
    out = set()
    for t in range(THREADS):
        chosen = excl[t] <= rank <= incl[t] if bug == "select_le" else excl[t] < rank <= incl[t]
        if n_valid > 0 and chosen:
            cum = 0 if bug == "thread_base" else excl[t]
            for k in range(BOX_PER):
                cum += hist[t * BOX_PER + k]
                if cum > rank if bug == "walk_gt" else cum >= rank:
                    out.add(t * BOX_PER + k)
                    break
    return n_valid, sorted(out)


def box_near_model(hist, median, band, bug=None):
    q = np.arange(BOX_BINS)
    return int(hist[(np.abs(q - median) < band) if bug == "band_lt" else (np.abs(q - median) <= band)].sum())


BOX_SUM_WIDTHS = (1, 2, 255, 256, 257, 511, 512, 513)
BOX_SUM_ROWS = (1, 3)
BOX_SUM_WHERE = ("last", "first", "every")


def box_sum_map(width, rows, where):
    """(d float32 [rows + 1, width + 1], box): valid pixels - seeded disparities 2 .. 60 in quarter pixels, all of them within the band 4
    of 30 where "near" is to select them - in the box's last column only, in column 0 only, or in every column; the map's last row
    and column, which no box holds, are valid too."""
    rng = np.random.default_rng(1000 * width + 10 * rows + len(where))
    d = (rng.integers(116, 125, (rows + 1, width + 1)) / 4.0).astype(np.float32)
    keep = np.zeros(d.shape, bool)
    keep[:, {"last": width - 1, "first": 0, "every": slice(None)}[where]] = True
    keep[rows, :], keep[:, width] = True, True
    return np.where(keep, d, np.float32(-1)), (0, 0, width, rows)


def box_sum_model(P, sel, bug=None):
    """k_box_positions' sums on the box's points P [rows, cols, 3] (sel bool [rows, cols]): a lane per column adds its rows top down
    onto +0.0, lanes 0 .. 2 add the column sums of each chunk of 256 left to right onto the running total."""
    assert bug is None or bug in BOX_SUM_BUGS
    rows, cols = P.shape[:2]
    col = np.zeros((cols, 3))
    for j in range(rows):
        col = np.where(sel[j][:, None], col + P[j], col)
    acc = np.zeros(3)
    for c0 in range(0, cols, THREADS):
        if bug == "chunk_carry":
            acc = np.zeros(3)
        n = min(cols - c0, THREADS) - (1 if bug == "last_column" else 0)
        for k in (range(n - 1, -1, -1) if bug == "right_to_left" else range(1 if bug == "first_column" and c0 == 0 else 0, n)):
            acc = acc + col[c0 + k]
    return acc


# ---------------------------------------------------------------------------------------------------------------- ground

GROUND_BINS = (8, 255, 256, 257, 511, 512, 513, 4081, 4095, 4096)
GROUND_BUGS = ("wave_base", "thread_base", "hi_clamp", "total_word", "tie_larger", "search_later_trips", "search_last_wave", "pick_later_trips", "rows_later_trips")

GroundCase = collections.namedtuple("GroundCase", "name d spec must")


def ground_row(masses, width, fill=-1.0):
    """float32 [width]: masses = [(bin or a disparity as float, pixels)], a bin b as b / 4 (0.0625 for bin 0), the rest of the row not valid."""
    row = []
    for b, n in masses:
        row += [(float(b) if isinstance(b, float) else (b / 4.0 if b > 0 else 0.0625))] * n
    assert len(row) <= width
    return np.array(row + [fill] * (width - len(row)), np.float32)


def ground_prefix_model(hist_row, bug=None):
    """k_ground_hist's in-place scan of one row's bins -> int64 [n_bins + 1], the words it stores: the exclusive prefix sums and the total."""
    h = np.asarray(hist_row, np.int64)
    n_bins = len(h)
    per = (n_bins + THREADS - 1) // THREADS
    lo = np.minimum(np.arange(THREADS) * per, n_bins)
    hi = np.minimum(lo + per, n_bins - 1 if bug == "hi_clamp" else n_bins)
    own = np.array([h[a:b].sum() for a, b in zip(lo, hi)], np.int64)
    excl, total = _wave_exclusive(own, bug == "wave_base")
    if bug == "thread_base":
        excl = np.repeat(excl[::64], 64)
    p = np.concatenate([h, [0 if bug == "total_word" else total]])  # a bin no thread scans keeps its count
    for t in range(THREADS):
        run = excl[t]
        for j in range(lo[t], hi[t]):
            p[j], run = run, run + h[j]
    return p


def ground_model(sv, d, spec, bug=None):
    """(vh, qb, S, n_valid) of one map as k_ground_hist, k_ground_search and k_ground_pick compute it, with 32-bit words where they do."""
    assert bug is None or bug in GROUND_BUGS
    d = np.asarray(d, np.float32)
    H = d.shape[0]
    p = sv.ground_params(H, **spec)
    n_bins, tol = p["n_bins"], p["tol"]
    P = np.stack([ground_prefix_model(r, bug) for r in sv.v_disparity(d, n_bins)])
    qbs = np.arange(p["qb_step"], n_bins, p["qb_step"], dtype=np.int64)
    n_qb = len(qbs)
    iq = np.arange(n_qb)
    best_keys = []
    for ivh, vh in enumerate(range(p["vh_lo"], p["vh_hi"] + 1, p["vh_step"])):
        den = H - 1 - vh
        S = np.zeros(n_qb, np.int64)
        for v in range(max(vh + 1, 0), H):
            ql = (2 * qbs * (v - vh) + den) // (2 * den)
            S = (S + P[v, np.minimum(ql + tol + 1, n_bins)] - P[v, np.maximum(ql - tol, 0)]) & 0xFFFFFFFF
        index = ivh * n_qb + iq
        keys = (S << 32) | (index if bug == "tie_larger" else 0xFFFFFFFF - index)
        live = np.ones(n_qb, bool)
        if bug == "search_later_trips":
            live &= iq < THREADS
        if bug == "search_last_wave":
            live &= (iq % THREADS) < 192
        best_keys.append(int(keys[live].max()) if live.any() else 0)
    if bug == "pick_later_trips":
        best_keys = best_keys[:THREADS]
    best = max(best_keys)
    S, low = best >> 32, best & 0xFFFFFFFF
    index = low if bug == "tie_larger" else 0xFFFFFFFF - low
    S = S - (1 << 32) if S >= 1 << 31 else S
    totals = P[:THREADS if bug == "rows_later_trips" else H, n_bins]
    found = S >= p["min_support"]
    return (p["vh_lo"] + (index // n_qb) * p["vh_step"] if found else -1, int(qbs[index % n_qb]) if found else -1, int(S), int(totals.sum()))


def ground_boundaries(n_bins):
    """name -> bin j: the boundaries j - 1 | j of the scan of n_bins bins - between the first two threads' runs, at the wavefront edges, at
    the last non-empty thread's (short) run, and the last bin."""
    per = (n_bins + THREADS - 1) // THREADS
    out = collections.OrderedDict()
    for name, j in (("thread_1", per), ("wave_1", 64 * per), ("wave_2", 128 * per), ("wave_3", 192 * per), ("last_thread", (n_bins - 1) // per * per), ("last_bin", n_bins - 1)):
        if 0 < j < n_bins:
            out[name] = j
    return out


def ground_boundary_cases(n_bins):
    """One frame of 2 rows per boundary: 5 pixels in bin j - 1 and 4 in bin j of the bottom row, 2 pixels of decoy in bin 1 (bin 6 where j
    is small) and, with tol 1, a window that takes both sides: S = 9 unless a prefix word is wrong.  In the last-bin frame the 4 pixels
    are +inf, 1e6 and the bin's own value, all of which the last bin takes; a frame more puts the window on the total word alone."""
    spec = dict(n_bins=n_bins, vh_lo=0, vh_hi=0, vh_step=1, qb_step=1, tol=1, min_support=0, min_run=1)
    per = (n_bins + THREADS - 1) // THREADS
    out = []
    for name, j in ground_boundaries(n_bins).items():
        last = j == n_bins - 1
        if last and name != "last_bin":
            continue  # the last thread's run is the last bin alone: the last-bin frames below
        decoy = 1 if j > 4 else 6
        top = [(INF, 2), (1e6, 1), (j, 1)] if last else [(j, 4)]
        d = np.stack([ground_row([(3, 1)], 12), ground_row([(j - 1, 5)] + top + [(decoy, 2)], 12)])
        base = "thread_base" if (j // per) % 64 else "wave_base"
        out.append(GroundCase("bins_%d_%s" % (n_bins, name), d, spec, ("hi_clamp", "total_word") if last else (base,)))
        if last:  # the last bin's own prefix word is read by the window of qb = n_bins - 1 at tol 0 alone: 5 pixels there, 4 beside it
            d = np.stack([ground_row([(3, 1)], 12), ground_row([(j - 1, 4), (INF, 2), (1e6, 2), (j, 1), (decoy, 2)], 12)])
            out.append(GroundCase("bins_%d_last_bin_alone" % n_bins, d, dict(spec, tol=0), ("hi_clamp", "total_word") + ((base,) if j % per == 0 else ())))
    return out


def ground_tie_cases():
    out = []
    flat = dict(vh_lo=0, vh_hi=0, vh_step=1, qb_step=1, tol=1, min_support=0, min_run=1)
    out.append(GroundCase("all_invalid", np.stack([ground_row([], 8), ground_row([], 8, fill=NAN)]), dict(flat, n_bins=64, vh_lo=-3, qb_step=2), ()))
    # one bin q* of the bottom row: every vh and every qb within tol of q* tie
    for n_qb, stars in ((255, (64,)), (256, (64,)), (257, (64, 256)), (600, (64, 256, 520))):
        for star in stars:
            d = np.stack([ground_row([], 4), ground_row([(star, 3)], 4)])
            must = ("tie_larger",) + (("search_later_trips",) if star > 257 else ())
            out.append(GroundCase("tie_qb_%d_at_%d" % (n_qb, star), d, dict(flat, n_bins=n_qb + 1, vh_lo=-2), must))
    for n_vh in (255, 256, 257, 600):
        d = np.stack([ground_row([], 4), ground_row([(5, 3)], 4)])
        out.append(GroundCase("tie_vh_%d" % n_vh, d, dict(flat, n_bins=8, vh_lo=1 - n_vh), ("tie_larger",)))
    # by exactly 1: a candidate of the second trip over one of the first; the best of wavefront 3 over the best of wavefront 0
    d = np.stack([ground_row([], 8), ground_row([(300, 4), (40, 3)], 8)])
    out.append(GroundCase("second_trip_by_one", d, dict(flat, n_bins=601, tol=0), ("search_later_trips",)))
    d = np.stack([ground_row([], 8), ground_row([(200, 4), (10, 3)], 8)])
    out.append(GroundCase("wave_3_by_one", d, dict(flat, n_bins=256, tol=0), ("search_last_wave",)))
    # the horizon row of the second / third trip of k_ground_pick's loop wins by exactly 1: vh = 0 alone sends row 1 to bin (100 + 1) // 2
    for n_vh in (257, 600):
        d = np.stack([ground_row([], 4), ground_row([(50, 1)], 4), ground_row([(100, 3)], 4)])
        out.append(GroundCase("pick_trip_by_one_%d" % n_vh, d, dict(flat, n_bins=128, tol=0, vh_lo=1 - n_vh, vh_hi=0), ("pick_later_trips",)))
    # k_ground_pick's row totals: a pixel per row, every seventh row without one
    for H in (257, 513):
        col = np.where(np.arange(H) % 7 == 3, -1.0, 0.5 + (np.arange(H) % 5) / 4.0).astype(np.float32)[:, None]
        out.append(GroundCase("rows_%d" % H, col, dict(n_bins=8, vh_lo=H - 40, vh_step=3, qb_step=1, tol=1, min_support=0, min_run=1), ("rows_later_trips",)))
    return out


# ---------------------------------------------------------------------------------------------------------------- cloud tile scan

CLOUD_Q = np.array([[0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])  # P = (d, d, d)
CLOUD_CROP = dict(lo=(0.0, 0.0, 0.0), hi=(4096.0,) * 3)
CLOUD_TILES = (1, 2, 255, 256, 257, 258, 511, 512, 513)
CLOUD_PATTERNS = ("last_tile", "tile_0", "index_mod_5", "full")
CLOUD_BUGS = ("wave_base", "thread_base", "hi_clamp", "total_without_wave_0", "capacity_plus_one")

CloudCase = collections.namedtuple("CloudCase", "name n_visited tile pattern step")


def cloud_cases(tile):
    """Every n_tiles x pattern on exactly n_tiles * tile visited pixels; one pixel less and one more around 256 and 512 tiles; the
    257-tile case on the lattice of step 2."""
    out = [CloudCase("%s_%d" % (p, n), n * tile, tile, p, 1) for n in CLOUD_TILES for p in CLOUD_PATTERNS]
    out += [CloudCase("%s_%d%+d" % (p, n, e), n * tile + e, tile, p, 1) for n in (256, 512) for p in ("index_mod_5", "full") for e in (-1, 1)]
    out += [CloudCase("%s_257_step2" % p, 257 * tile, tile, p, 2) for p in ("index_mod_5", "full")]
    return out


def cloud_keep(case):
    """bool [n_visited]: the visited pixels the pattern keeps - the first k pixels of a tile that holds k points."""
    v = np.arange(case.n_visited)
    t, o = v // case.tile, v % case.tile
    last = (case.n_visited - 1) // case.tile
    return {"last_tile": t == last, "tile_0": t == 0, "index_mod_5": o < t % 5, "full": np.ones(len(v), bool)}[case.pattern]


def cloud_map(case):
    """float32 [1, W]: 1 + (v % 997) / 8 at a kept visited pixel v, -1 at the others; with a step the pixels between the visited ones are valid."""
    keep = cloud_keep(case)
    d = np.full((1, (case.n_visited - 1) * case.step + 1), 3.0, np.float32)
    d[0, ::case.step] = np.where(keep, 1.0 + (np.arange(case.n_visited) % 997) / 8.0, -1.0)
    return d


def cloud_scan_model(tile_counts, bug=None):
    """k_cloud_scan on a frame's tile counts -> (the offset of every tile, the count)."""
    assert bug is None or bug in CLOUD_BUGS
    c = np.asarray(tile_counts, np.int64)
    n = len(c)
    per = (n + THREADS - 1) // THREADS
    lo = np.minimum(np.arange(THREADS) * per, n)
    hi = np.minimum(lo + per, n - 1 if bug == "hi_clamp" else n)
    own = np.array([c[a:b].sum() for a, b in zip(lo, hi)], np.int64)
    excl, total = _wave_exclusive(own, bug == "wave_base")
    if bug == "thread_base":
        excl = np.repeat(excl[::64], 64)
    if bug == "total_without_wave_0":
        total -= int(own[:64].sum())
    out = c.copy()  # a tile no thread scans keeps its count
    for t in range(THREADS):
        run = excl[t]
        for k in range(lo[t], hi[t]):
            out[k], run = run, run + c[k]
    return out, (total if bug == "total_without_wave_0" else int(excl[255] + own[255]))


def cloud_rows_model(case, capacity, bug=None):
    """(index int64 [rows], count): the pixel index k_cloud_write stores in every row below the capacity, POISON where none lands; a later
    tile overwrites an earlier one where a wrong offset makes them meet."""
    keep = cloud_keep(case)
    tiles = -(-case.n_visited // case.tile)
    counts = np.bincount(np.nonzero(keep)[0] // case.tile, minlength=tiles)
    offset, count = cloud_scan_model(counts, bug)
    cap = capacity + (1 if bug == "capacity_plus_one" else 0)
    rows = np.full(max(min(int(keep.sum()), capacity), 0) + 2 * case.tile, POISON, np.int64)
    kept = np.nonzero(keep)[0]
    rank = np.arange(len(kept)) - np.searchsorted(kept // case.tile, kept // case.tile)  # inside its tile
    row = offset[kept // case.tile] + rank
    ok = (row < cap) & (row < len(rows))
    rows[row[ok]] = kept[ok] * case.step
    n = len(rows)
    while n and rows[n - 1] == POISON:
        n -= 1
    return rows[:n], count


# ---------------------------------------------------------------------------------------------------------------- voxel row ranks

VOXEL_RANK_GRID = dict(size=1.0 / 32, lo=(0.0, 0.0, 0.0), hi=(64.0, 64.0, 64.0))  # 2048 cells an axis: visited pixel v alone in cell (v, v, v)
VOXEL_PATTERNS = ("lane_63", "lane_0", "bit_per_lane", "all", "nothing")
VOXEL_BUGS = ("lane_base", "tile_offset", "inclusive")


def voxel_owner_bits(pattern, tiles, tile):
    """bool [tiles * tile]: the visited pixels that are kept - each the owner of a voxel of its own; lane L of a tile's wavefront holds the
    16 pixels 16 L .. 16 L + 15."""
    o = np.arange(tile)
    one = {"lane_63": o >= tile - 16, "lane_0": o < 16, "bit_per_lane": o % 16 == (o // 16) % 16, "all": np.ones(tile, bool), "nothing": np.zeros(tile, bool)}[pattern]
    return np.tile(one, tiles)


def voxel_rank_map(pattern, tiles, tile):
    """float32 [1, tiles * tile]: (v + 0.5) / 32 at a kept visited pixel v - cell v on all three axes under CLOUD_Q and VOXEL_RANK_GRID -,
    -1 at the others."""
    keep = voxel_owner_bits(pattern, tiles, tile)
    return np.where(keep, (np.arange(len(keep)) + 0.5) / 32.0, -1.0).astype(np.float32)[None]


def voxel_rows_model(keep, tile, bug=None):
    """int64 [rows]: the pixel k_voxel_write stores as `first` in every row: the tile's offset + the owners in the lanes below + the
    owners below inside the lane's 16 bits; a later lane overwrites an earlier one where a wrong rank makes them meet."""
    assert bug is None or bug in VOXEL_BUGS
    keep = np.asarray(keep, bool)
    rows = np.full(2 * len(keep) + 32, POISON, np.int64)
    offset = 0
    for t in range(len(keep) // tile):
        bits = keep[t * tile:(t + 1) * tile].reshape(64, 16)
        own = bits.sum(1)
        incl = np.cumsum(own)
        for lane in range(64):
            r = (0 if bug == "tile_offset" else offset) + (0 if bug == "lane_base" else incl[lane] - (0 if bug == "inclusive" else own[lane]))
            for k in np.nonzero(bits[lane])[0]:
                rows[r] = t * tile + lane * 16 + k
                r += 1
        offset += int(own.sum())
    n = len(rows)
    while n and rows[n - 1] == POISON:
        n -= 1
    return rows[:n]
