"""Inputs for a voxel map re-posed under per-frame rigid corrections (group (AD)).  A case is a dict: dst and src, each (params, calls) as
voxel_map_cases has them; corr float64 [K,12]; kw - seq0 and the filters of voxel_map_repose -; and optionally src_seq0 (the sequence
number of src's first frame), carve (frames and keywords of a voxel_map_carve run on src before the re-pose, which leaves tombstones) and
loose (dst overflows during the call: its content and `claimed` are undefined, the flag and the other counts are not).

The rounding cases are solved, not drawn: per voxel a correction whose translation puts the transformed centre within a few ulps of a
cell edge or of an offset step of the destination, kept only where a named mistake - a fused multiply-add in the transform, a
multiplication by 1 / size in place of the division, the centre formed as S / n first - changes the cell or the offset."""
from fractions import Fraction

import numpy as np

import voxel_carry_cases as carry
import voxel_map_cases as cases
from voxel_map_cases import BOX16, IDENTITY

STATS = ("carried", "filtered", "outside", "claimed")
BOX = dict(lo=(-8.0, -8.0, -2.0), hi=(8.0, 8.0, 2.0), size=0.5, capacity=4096)       # 32 x 32 x 8 cells
OTHER = dict(lo=(-6.1, -7.3, -1.45), hi=(9.2, 6.4, 2.35), size=0.3, capacity=8192)   # another box, size and capacity
SEQ_MAX = 2 ** 31 - 2


def rigid(rng, angle=0.05, shift=0.4):
    """A small random rigid motion as twelve words: Rodrigues' formula about a random axis."""
    om = rng.uniform(-1, 1, 3)
    om *= rng.uniform(0, angle) / np.sqrt((om * om).sum())
    a = np.sqrt((om * om).sum())
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    R = np.eye(3) + (np.sin(a) / a) * K + ((1.0 - np.cos(a)) / (a * a)) * (K @ K)
    return np.concatenate([R.reshape(9), rng.uniform(-shift, shift, 3)])


def cloud(box, B, rows, seed, weights=(1, 9), inside=0.95):
    """One call of B frames of `rows` random rows inside the middle of `box`, with colours and weights."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(box["lo"]), np.array(box["hi"])
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * inside
    xyz = mid + rng.uniform(-1, 1, (B, rows, 3)) * half
    return (xyz, rng.integers(0, 256, (B, rows, 4)).astype(np.uint8), rng.integers(weights[0], weights[1] + 1, (B, rows)).astype(np.int32),
            np.full(B, rows, np.int32), np.tile(IDENTITY, (B, 1)))


def to_point(p):
    """The correction with R = 0 and t = p: every voxel goes to p."""
    return np.concatenate([np.zeros(9), np.asarray(p, np.float64)])


# ------------------------------------------------------------------------------------------------------------------ rounding edges

def fma(a, b, c):
    """a * b + c rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def centre(lo, size, c, S, n, first_quotient=False):
    """The read-out's centre on one axis, as written; first_quotient: the mistake that forms S / n first."""
    if first_quotient:
        return lo + (float(c) + (float(S) / float(n) + 0.5) / 65536.0) * size
    return lo + (float(c) + (float(S) + 0.5 * float(n)) / (65536.0 * float(n))) * size


def world(w, k, p, fused=False):
    """The insert's transform on axis k, as written; fused: the mistake of a compiler that contracts."""
    if fused:
        return fma(w[3 * k + 2], p[2], fma(w[3 * k + 1], p[1], w[3 * k] * p[0])) + w[9 + k]
    return ((w[3 * k] * p[0] + w[3 * k + 1] * p[1]) + w[3 * k + 2] * p[2]) + w[9 + k]


def cell_of(box, k, P, reciprocal=False):
    """(c, u) of the coordinate P on axis k of `box`, or None outside; reciprocal: the mistake of multiplying by 1 / size."""
    if not (box["lo"][k] < P < box["hi"][k]):
        return None
    t = (P - box["lo"][k]) * (1.0 / box["size"]) if reciprocal else (P - box["lo"][k]) / box["size"]
    c = min(int(t), cases._cells(box)[k] - 1)
    return c, min(int((t - float(c)) * 65536.0), 65535)


MISTAKES = ("fused", "reciprocal", "first_quotient")


def landing(src_box, dst_box, key, S, n, w, mistake=None):
    """[(c, u) or None per axis] of the voxel (key, S, n) of src_box under the correction w in dst_box, under one mistake or none."""
    p = [centre(src_box["lo"][k], src_box["size"], (key >> (20 * k)) & 0xFFFFF, S[k], n, mistake == "first_quotient") for k in range(3)]
    return [cell_of(dst_box, k, world(w, k, p, mistake == "fused"), mistake == "reciprocal") for k in range(3)]


def rounding_case(want=16, seed=91):
    """-> (case, found): `want` voxels, one per frame, each with a correction of its own solved onto a cell edge or an offset step of
    OTHER; found[v] = the mistakes that move voxel v.  Every mistake of MISTAKES moves at least one of them."""
    rng = np.random.default_rng(seed)
    # Boxes that start near 0, so that one ulp of the centre survives lo + . and P - lo; a size of the destination whose reciprocal is
    # not exact enough to stand in for the division (0.3's is: the two never differ).
    src_box = dict(lo=(-0.05, -0.03, -0.02), hi=(5.55, 5.57, 2.08), size=0.35, capacity=512)
    dst_box = dict(lo=(-0.07, -0.11, -0.09), hi=(8.93, 8.89, 3.51), size=0.45, capacity=512)
    src_cells, lo, size = cases._cells(src_box), src_box["lo"], src_box["size"]
    frames, corr, found, used = [], [], [], set()
    per = {m: 0 for m in MISTAKES}
    for _ in range(4000):
        if len(frames) >= want and all(v >= 3 for v in per.values()):
            break
        k = int(rng.integers(0, 3))  # the axis that is solved
        c = [int(rng.integers(0, 4)) for _ in range(3)]
        rows = np.array([[lo[a] + (c[a] + rng.uniform(0.05, 0.95)) * size for a in range(3)] for _ in range(2)])
        if rng.integers(0, 2):  # S / n just below a power of two in cell 0 of that axis: (S / n) + 0.5 then rounds where (S + 0.5 n) / n does not
            c[k] = 0
            j = int(rng.integers(11, 16))
            rows[:, k] = [lo[k] + (((2 ** j - 1 + r) + 0.5) / 65536.0) * size for r in range(2)]
        wts = rng.integers(1, 1000, 2)
        keyed = [cases.row_key(src_box, r, [float(v) for v in IDENTITY], int(wt)) for r, wt in zip(rows, wts)]
        if any(r is None for r in keyed) or keyed[0][0] != keyed[1][0] or keyed[0][0] in used:  # a voxel of its own per frame
            continue
        wts.sort()  # the heavier row second: the mean lies in the upper half between the two
        key, n = keyed[0][0], int(wts.sum())
        S = [int(wts[0]) * keyed[0][1][k] + int(wts[1]) * keyed[1][1][k] for k in range(3)]
        w = [float(v) for v in rigid(rng, 0.3, 0.2)]
        p = [centre(lo[k], size, c[k], S[k], n) for k in range(3)]
        # the target: a cell edge of dst (every third) or an offset step inside a cell, near where the voxel lands anyway
        here = world(w, k, p)
        cs = int((here - dst_box["lo"][k]) / dst_box["size"])
        step = 0 if rng.integers(0, 3) == 0 else int(rng.integers(1, 65536))
        target = dst_box["lo"][k] + (cs + step / 65536.0) * dst_box["size"]
        w[9 + k] += target - here
        base = w[9 + k]
        hit = None
        for d in sorted(range(-8, 9), key=abs):  # the first step that a mistake not seen so far moves; else the first that any moves
            w[9 + k] = base + d * float(np.spacing(target))  # steps of the coordinate's ulp, which is coarser than the translation's
            right = landing(src_box, dst_box, key, S, n, w)
            if any(r is None for r in right):
                continue
            moved = [m for m in MISTAKES if landing(src_box, dst_box, key, S, n, w, m) != right]
            fresh = any(per[m] < 3 for m in moved)
            if moved and (fresh or (hit is None and len(frames) < want)):
                hit = (d, moved)
                if fresh:
                    break
        if hit is None:
            continue
        w[9 + k] = base + hit[0] * float(np.spacing(target))
        for m in hit[1]:
            per[m] += 1
        frames.append((rows, wts))
        used.add(key)
        corr.append(list(w))
        found.append(hit[1])
    assert len(frames) >= want and all(v >= 3 for v in per.values()), (len(frames), per)
    B = len(frames)
    xyz = np.stack([f[0] for f in frames])
    call = (xyz, None, np.stack([f[1] for f in frames]).astype(np.int32), np.full(B, 2, np.int32), np.tile(IDENTITY, (B, 1)))
    return dict(dst=(dst_box, []), src=(src_box, [call]), corr=np.array(corr), kw={}), found


# ------------------------------------------------------------------------------------------------------------------ cases

def repose_cases():
    """{name: case}, shared by the CPU tests (the numpy form against the plain loop) and the GPU tests (the device against the numpy form)."""
    rng = np.random.default_rng(17)
    out = {}
    src8 = (BOX, [cloud(BOX, 8, 300, 1)])  # about 2 000 voxels from rows of 8 frames
    small8 = np.array([rigid(rng) for _ in range(8)])
    empty = (BOX, [])
    # 1. several frames, several corrections
    out["frames_8"] = dict(dst=empty, src=src8, corr=small8, kw={})
    out["identity"] = dict(dst=empty, src=src8, corr=IDENTITY[None], kw={})
    # 2. the smallest table a map admits (1 024 slots), and one the walk needs two strides for (2^20 slots, 4 096 tiles of 2 048 workgroups)
    out["table_smallest"] = dict(dst=empty, src=(dict(BOX, capacity=512), [cloud(BOX, 2, 100, 2)]), corr=small8[:2], kw={})
    out["table_two_strides"] = dict(dst=empty, src=(dict(BOX, capacity=2 ** 19), [cloud(BOX, 8, 300, 3)]), corr=small8, kw={})
    # 3. everything into one cell, 4. into four
    out["one_cell"] = dict(dst=empty, src=src8, corr=np.tile(to_point((1.3, -2.2, 0.6)), (8, 1)), kw={})
    four = [(1.3, -2.2, 0.6), (-7.9, 7.9, 1.9), (0.0, 0.0, 0.0), (1.3, -2.2, -0.6)]
    out["four_cells"] = dict(dst=empty, src=src8, corr=np.array([to_point(four[b % 4]) for b in range(8)]), kw={})
    out["one_cell_held"] = dict(dst=(BOX, [cloud(BOX, 1, 40, 4)[:4] + (to_point((1.3, -2.2, 0.6))[None],)]), src=src8, corr=np.tile(to_point((1.3, -2.2, 0.6)), (8, 1)), kw={})
    # 5. the index rule: both clamps, and sequence numbers at the top of their range
    out["index_clamps"] = dict(dst=empty, src=src8, corr=small8[:3], kw=dict(seq0=3))
    out["index_seq_top"] = dict(dst=empty, src=src8, src_seq0=SEQ_MAX - 7, corr=small8[:5], kw=dict(seq0=SEQ_MAX - 5))
    out["index_seq0_top"] = dict(dst=empty, src=src8, corr=small8[:5], kw=dict(seq0=SEQ_MAX))
    # 6. filters and invalid corrections
    thin = (BOX, [cloud(BOX, 8, 300, 5, weights=(1, 3), inside=0.5)])  # a denser cloud: voxels of several rows
    out["filter_min_n"] = dict(dst=empty, src=thin, corr=small8, kw=dict(min_n=4))
    out["filter_min_rows"] = dict(dst=empty, src=thin, corr=small8, kw=dict(min_rows=2))
    out["filter_since"] = dict(dst=empty, src=thin, corr=small8, kw=dict(since=5))
    out["filters_together"] = dict(dst=empty, src=thin, corr=small8, kw=dict(min_n=3, min_rows=2, since=2))
    line = (BOX16, [cases.one_frame(cases.cell_points([(x, 8, 8) for x in range(3, 13)] + [(x, 3, 3) for x in range(2, 9)]), np.full((17, 4), 90), np.arange(1, 18))])
    ray = (np.array([[[14.5, 8.5, 8.5]]]), np.array([[5]], np.int32), np.array([1], np.int32), IDENTITY[None])
    carve = dict(frames=ray, kw=dict(origin=(0.5, 8.5, 8.5), seq0=1, reach=16, margin=1, min_miss=1, ratio=0))
    for min_n in (1, 0):
        out["tombstones_min_n_%d" % min_n] = dict(dst=(BOX16, []), src=line, carve=carve, corr=small8[:1], kw=dict(min_n=min_n, min_rows=0))
    bad = small8.copy()
    bad[2, 4], bad[5, 10] = np.nan, np.inf
    bad[6, 0] = -np.inf
    out["not_finite"] = dict(dst=empty, src=src8, corr=bad, kw={})
    away = small8.copy()
    away[1, 9], away[4, 11], away[7, 9] = 100.0, -5.0, 1e300
    out["taken_outside"] = dict(dst=empty, src=src8, corr=away, kw={})
    # 7. a destination that holds voxels, with another box, another size and another capacity
    out["other_box"] = dict(dst=(OTHER, [cloud(OTHER, 3, 200, 6)]), src=src8, corr=small8, kw={})
    out["other_box_empty"] = dict(dst=(OTHER, []), src=src8, corr=small8, kw=dict(min_n=2))
    # 8. overflow: of src, of dst, and of dst during the call
    three = carry.frames([[(1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 77, 0)]], seed=6)
    some = (BOX16, [carry.frames([[(1, 1, 1), (2, 2, 2)], [(3, 3, 3)]], seed=2)])
    out["overflowed_source"] = dict(dst=some, src=(dict(BOX16, capacity=2), [three]), corr=small8[:1], kw={})
    out["overflowed_destination"] = dict(dst=(dict(BOX16, capacity=2), [three]), src=some, corr=small8[:1], kw={})
    out["overflows_meanwhile"] = dict(dst=(dict(BOX, capacity=512), []), src=src8, corr=small8, kw={}, loose=True)
    # 9. rounding edges
    out["rounding_edges"] = rounding_case()[0]
    return out


# ------------------------------------------------------------------------------------------------------------------ the loop scenario

DRIVE_BOX = dict(lo=(-5.0, -10.0, -1.0), hi=(50.0, 8.0, 4.0), size=0.25, capacity=2 ** 15)
DRIVE_FRAMES, DRIVE_PASS2 = 100, 60  # frames 0 .. 39 pass the street, 40 .. 59 see nothing, 60 .. 99 pass it again


def drive_surfaces():
    """float64 [N,3]: a wall along x at y = 3 and the faces of three boxes at y = -2.5, sampled every 0.1 m."""
    xs, zs = np.arange(0.0, 46.0, 0.1), np.arange(0.0, 2.0, 0.1)
    wall = np.stack(np.meshgrid(xs, [3.0], zs, indexing="ij"), -1).reshape(-1, 3)
    boxes = [np.stack(np.meshgrid(np.arange(bx, bx + 1.0, 0.1), [-2.5], np.arange(0.0, 1.0, 0.1), indexing="ij"), -1).reshape(-1, 3) for bx in (10.0, 21.0, 33.0)]
    return np.concatenate([wall] + boxes)


def drive_truth(sv):
    """The true poses [100,12]: two passes along x, the second 0.37 m ahead and 0.2 m to the side, a block driven round between them."""
    k = np.arange(DRIVE_FRAMES)
    x = np.where(k < 40, k * 1.0, np.where(k < DRIVE_PASS2, 39.0 - (k - 40) * 2.0, (k - DRIVE_PASS2) * 1.0 + 0.37))
    y = np.where(k < 40, 0.0, np.where(k < DRIVE_PASS2, -40.0, 0.2))
    return sv.voxel_map_pose(x, y, np.where((k >= 40) & (k < DRIVE_PASS2), np.pi, 0.01 * np.sin(k)))


def drive_frames(sv, truth):
    """One call: per frame the surface points 2 .. 5 m ahead of the vehicle, in the vehicle's axes (none between the passes)."""
    W = drive_surfaces()
    rows = []
    for k in range(DRIVE_FRAMES):
        if 40 <= k < DRIVE_PASS2:
            rows.append(np.zeros((0, 3)))
            continue
        inv = sv._pose_inv(truth[k])
        Pf = W @ inv[:9].reshape(3, 3).T + inv[9:]
        rows.append(Pf[(Pf[:, 0] >= 2.0) & (Pf[:, 0] <= 5.0)])
    cap = max(len(r) for r in rows)
    xyz = np.zeros((DRIVE_FRAMES, cap, 3))
    for k, r in enumerate(rows):
        xyz[k, :len(r)] = r
    return xyz, None, None, np.array([len(r) for r in rows], np.int32)


def strangers(state, truth_state, since):
    """(share, count): of the voxels of `state` with last_seq >= since, those in a cell that is neither a cell of truth_state nor
    26-adjacent to one."""
    def cells(key):
        return np.stack([key & 0xFFFFF, (key >> 20) & 0xFFFFF, (key >> 40) & 0xFFFFF], -1)
    near = set()
    for c in cells(truth_state["key"]).tolist():
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    near.add((c[0] + dx, c[1] + dy, c[2] + dz))
    late = cells(state["key"][(state["last_seq"] >= since) & (state["n"] >= 1)]).tolist()
    far = sum(tuple(c) not in near for c in late)
    return far / max(len(late), 1), len(late)
