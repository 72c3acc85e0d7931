"""Inputs of the place recognition tests (test_places.py): frames of rows that sit on the descriptor's cell rules, descriptor sets that
sit on the search's rules, and a synthetic town seen from many places.  Everything is made from seeds or by hand; nothing is measured
here."""
import math

import numpy as np

DESC_FIELDS = ("desc", "ring", "words")
SHARE = 64      # keys of a workgroup of the search (PLACE_SHARE)
CHUNK = 4096    # rows of a workgroup of the binning kernel (PLACE_CHUNK)


def same(got, want, fields):
    return all(np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.array_equal(np.asarray(got[k]), np.asarray(want[k])) for k in fields)


# ------------------------------------------------------------------------------------------------------------- descriptor

def frame(sv, rows, params, dtype=np.float64, n=None, counts=None, poses=None, cap=None):
    """One frame [1,cap,3] from a list of (x, y, z)."""
    rows = np.asarray(rows, np.float64).reshape(-1, 3)
    cap = len(rows) if cap is None else cap
    xyz = np.zeros((1, cap, 3), dtype)
    xyz[0, :len(rows)] = rows
    return {"xyz": xyz, "n": n, "counts": np.array([len(rows)], np.int32) if counts is None else counts, "params": params, "poses": poses}


def at_cell(params, qx, qy, z=1.0):
    """A row in the middle of cell (qx, qy): floor(x / unit) = qx whatever the last bit."""
    return ((qx + 0.5) * params["unit"], (qy + 0.5) * params["unit"], z)


def sector_boundaries(sv, S):
    """q on the boundary of every sector - the integer points nearest to a multiple of dir[k], and the exact multiples where dir[k] has a
    short integer form - and the eight cells around each."""
    p = sv.place_params(30.0, rings=4, sectors=S)
    rows = []
    for dx, dy in p["dirs"].tolist():
        g = math.gcd(abs(dx), abs(dy))
        exact = [(dx // g * t, dy // g * t) for t in (1, 2, 400)] if max(abs(dx), abs(dy)) // g <= 2 else []
        near = [(int(np.rint(dx * t / 16384.0)), int(np.rint(dy * t / 16384.0))) for t in (3, 300, 700, 1020)]
        for qx, qy in exact + near:
            rows += [at_cell(p, qx + ex, qy + ey) for ex in (-1, 0, 1) for ey in (-1, 0, 1)]
    return frame(sv, rows, p)


def ring_edges(sv):
    """d2 just below, at and just above every ring edge, r_min2 and 1024^2: the cells whose d2 is the nearest sum of two squares."""
    p = sv.place_params(30.0, rings=20, sectors=8, r_min=3.0)
    q = np.arange(0, 1026, dtype=np.int64)
    d2 = (q[:, None] ** 2 + q[None, :] ** 2)
    flat = np.sort(np.unique(d2))
    rows = []
    for e2 in sorted(set(p["ring_edge2"].tolist() + [p["r_min2"], 1024 * 1024])):
        at = np.searchsorted(flat, e2)
        for v in flat[max(at - 1, 0):at + 2]:
            qx, qy = np.argwhere(d2 == v)[0]
            rows += [at_cell(p, int(qx), int(qy)), at_cell(p, -int(qy) - 1, int(qx)), at_cell(p, -int(qx) - 1, -int(qy) - 1)]
    return frame(sv, [r for r in rows if abs(r[0]) < 31 and abs(r[1]) < 31], p)


def height_edges(sv, dtype):
    p = sv.place_params(30.0, rings=4, sectors=8)
    t = np.dtype(dtype).type
    zs = [p["z_lo"], np.nextafter(t(p["z_lo"]), t(-np.inf)), np.nextafter(t(p["z_lo"]), t(np.inf)), p["z_hi"], np.nextafter(t(p["z_hi"]), t(-np.inf)),
          p["z_lo"] + 254 * p["z_unit"], p["z_lo"] + 255 * p["z_unit"], np.nextafter(p["z_lo"] + 254 * p["z_unit"], -np.inf)]
    zs += [p["z_lo"] + k * p["z_unit"] for k in range(1, 254, 23)]
    return frame(sv, [at_cell(p, 100 + 7 * i, 50 - 11 * i, float(z)) for i, z in enumerate(zs)], p, dtype)


def near_integers(sv):
    """x with x / unit within an ulp of an integer m, for every m: m unit and its neighbours in double.  -> (the frame, how many of
    them a multiplication by 1 / unit puts into another cell than the division)."""
    p = sv.place_params(30.0, rings=4, sectors=8)
    unit = np.float64(p["unit"])
    m = np.arange(-1023, 1024, dtype=np.float64)
    x = np.concatenate([m * unit, np.nextafter(m * unit, -np.inf), np.nextafter(m * unit, np.inf)])
    differ = int((np.floor(x / unit) != np.floor(x * (np.float64(1.0) / unit))).sum())
    rows = np.stack([x, np.roll(x, 977), np.ones_like(x)], -1)
    return frame(sv, rows, p), differ


def random_frames(sv, seed, B, cap, dtype=np.float32, poses=False, params=None, bad=True):
    """Frames of random rows, some outside every rule, some not finite, some with n = 0; counts of 0 and -1 and above cap among them; the
    rows behind counts hold garbage."""
    rng = np.random.default_rng(seed)
    p = params or sv.place_params(30.0)
    xyz = rng.uniform(-33, 33, (B, cap, 3))
    xyz[..., 2] = rng.uniform(p["z_lo"] - 0.5, p["z_hi"] + 0.5, (B, cap))
    xyz = xyz.astype(dtype)
    n = rng.integers(-1, 4, (B, cap)).astype(np.int32)
    counts = rng.integers(max(cap // 2, 1), cap + 1, B).astype(np.int32)
    if bad:
        sick = rng.random((B, cap)) < 0.05
        xyz[sick, rng.integers(0, 3, int(sick.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(sick.sum()))
        if B >= 3:
            counts[1], counts[2] = 0, -1
        if B >= 5:
            counts[4] = cap + 7
        for b in range(B):
            xyz[b, max(int(counts[b]), 0):] = np.nan if b % 2 else 1.0e30
    P = None
    if poses:
        P = sv.voxel_render_cams(sv.voxel_map_pose(rng.uniform(-3, 3, B), rng.uniform(-3, 3, B), rng.uniform(-3.2, 3.2, B), rng.uniform(-0.2, 0.2, B)))
    return {"xyz": xyz, "n": n, "counts": counts, "params": p, "poses": P}


def descriptor_cases(sv):
    """name -> arguments: what the CPU tests hold against the brute form and the GPU tests against the numpy form."""
    cases = {"sectors8": sector_boundaries(sv, 8), "sectors60": sector_boundaries(sv, 60), "rings": ring_edges(sv), "z64": height_edges(sv, np.float64),
             "z32": height_edges(sv, np.float32), "near": near_integers(sv)[0]}
    for cap in (1, 63, 64, 65, CHUNK + 1):
        cases["cap%d" % cap] = random_frames(sv, cap, 3, cap, np.float32 if cap % 2 else np.float64, poses=cap in (64, CHUNK + 1))
    for B in (1, 65):
        cases["B%d" % B] = random_frames(sv, 100 + B, B, 40, np.float64 if B == 1 else np.float32, poses=B == 65)
    cases["wide"] = random_frames(sv, 5, 2, 300, params=sv.place_params(25.0, rings=32, sectors=128, z_lo=-1.0, z_hi=3.0, r_min=2.0))
    cases["tall"] = random_frames(sv, 6, 2, 300, np.float64, poses=True, params=sv.place_params(40.0, rings=64, sectors=64))
    return cases


def call_descriptor(f, case, **extra):
    return f(case["xyz"], case["n"], case["counts"], case["params"], case["poses"], **extra)


# ------------------------------------------------------------------------------------------------------------- search

MATCH_FIELDS = ("best", "counts")


def described(desc):
    """words and ring of descriptors [N,R,S] as place_descriptor would give them (kept = the occupied bins, dropped = 0)."""
    desc = np.ascontiguousarray(desc, np.uint8)
    occ = (desc > 0).sum(2)
    words = np.stack([desc.astype(np.int64).sum((1, 2)), occ.sum(1), occ.sum(1), np.zeros(len(desc), np.int64)], -1).astype(np.int32)
    return desc, words, occ.astype(np.uint8)


def match_case(q, k, q_seq=None, k_seq=None, min_gap=0, **words):
    q = np.asarray(q, np.uint8)
    qd, qw, qr = described(q[None] if q.ndim == 2 else q)  # one descriptor [R,S] is one query
    kd, kw, kr = described(np.asarray(k, np.uint8).reshape((-1,) + qd.shape[1:]))
    q_seq = np.full(len(qd), 10 ** 6, np.int32) if q_seq is None else np.asarray(q_seq, np.int32)
    k_seq = np.arange(len(kd), dtype=np.int32) if k_seq is None else np.asarray(k_seq, np.int32)
    return {"args": (qd, qw, qr, q_seq, kd, kw, kr, k_seq, min_gap), "words": words}


def call_match(f, case, **extra):
    return f(*case["args"], **case["words"], **extra)


def row8(*v):
    """A descriptor [1,8] from its first values."""
    return np.array([list(v) + [0] * (8 - len(v))], np.uint8)


def random_match(seed, Q, K, R, S, **words):
    """Sparse random keys; every query is a key rolled and disturbed; sequence numbers on both sides of the queries'."""
    rng = np.random.default_rng(seed)
    k = (rng.integers(1, 256, (K, R, S)) * (rng.random((K, R, S)) < 0.3)).astype(np.uint8)
    q = np.zeros((Q, R, S), np.uint8)
    for i in range(Q):
        q[i] = np.roll(k[rng.integers(0, K)], rng.integers(0, S), axis=1) if K else rng.integers(0, 256, (R, S))
        hit = rng.random((R, S)) < 0.1
        q[i][hit] = rng.integers(0, 256, int(hit.sum()))
    return match_case(q, k, rng.integers(40, 60, Q), rng.integers(0, 100, K), **words)


def match_cases():
    """name -> case.  The hand-made ones say in test_places.py what must come out."""
    c = {}
    for K in (0, 1, SHARE - 1, SHARE, SHARE + 1):
        c["K%d" % K] = random_match(K, 5 if K == SHARE + 1 else 1, K, 3, 60, min_gap=3, ring_gate=-1 if K % 2 else 40)
    for S in (8, 60, 64, 68, 128):
        c["S%d" % S] = random_match(200 + S, 2, 9, 2, S, min_gap=0)
    c["R1"] = random_match(31, 5, 70, 1, 128, min_gap=5, ring_gate=6)
    c["R64"] = random_match(32, 1, 5, 64, 64, min_gap=0)
    for ms in (0, 1, 30):
        c["max_shift%d" % ms] = random_match(40, 3, 20, 2, 60, min_gap=0, max_shift=ms)
    c["full"] = match_case(np.full((1, 32, 128), 255, np.uint8), np.full((2, 32, 128), 1, np.uint8))  # sad 254 * 4096: the word's width
    c["constant"] = match_case(np.full((1, 2, 60), 9, np.uint8), np.full((3, 2, 60), 7, np.uint8))    # every shift ties, duplicate keys
    c["tie"] = match_case(row8(5), np.stack([row8(4, 4, 1), row8(2)]))        # 6 / 14 against 3 / 7: the lower index
    c["tie_swapped"] = match_case(row8(5), np.stack([row8(2), row8(4, 4, 1)]))
    c["close"] = match_case(row8(5), np.stack([row8(3, 3), row8(2)]))         # 5 / 11 against 3 / 7: 33 < 35
    wide = np.full((2, 32, 128), 100, np.uint8)
    wide[1, 7, 9] = 102
    c["cross64"] = match_case(np.full((1, 32, 128), 200, np.uint8), wide)     # 409600 / 1228800 against 409598 / 1228802: products of 2^39
    c["gap"] = match_case(row8(5), np.stack([row8(5)] * 5), q_seq=[10], k_seq=[7, 13, 10, 8, 12], min_gap=3)
    c["gate_at"] = match_case(np.array([[[3, 0, 0, 0, 0, 0, 0, 0], [0] * 8]], np.uint8), np.array([[[3, 1, 0, 0, 0, 0, 0, 0], [2] + [0] * 7]], np.uint8), ring_gate=2)
    c["gate_below"] = dict(c["gate_at"], words={"ring_gate": 1})
    c["accept_at"] = match_case(row8(5), row8(11)[None], accept=96)           # 256 * 6 = 96 * 16
    c["accept_below"] = match_case(row8(5), row8(11)[None], accept=95)
    c["empty_query"] = match_case(np.stack([row8(), row8(5)]), np.stack([row8(5), row8(6)]))
    c["empty_key"] = match_case(row8(5), np.stack([row8(), row8(9), row8(), row8(5)]))
    return c


# ------------------------------------------------------------------------------------------------------------- a town

TOWN_SIDE = 160.0   # metres
TOWN_R_MAX = 30.0


def town(seed):
    """Walls and boxes as rows [N,3] in the world: the upper edges of random blocks, a point every half metre, and four long walls."""
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(260):
        cx, cy = rng.uniform(0, TOWN_SIDE, 2)
        w, d, h = rng.uniform(1, 7), rng.uniform(1, 7), rng.uniform(0.3, 4.2)
        yaw = rng.uniform(0, np.pi)
        for side in range(4):
            a = np.arange(0, (w, d)[side % 2], 0.5)
            u, v = ((a - w / 2, np.full_like(a, -d / 2)), (np.full_like(a, w / 2), a - d / 2), (w / 2 - a, np.full_like(a, d / 2)), (np.full_like(a, -w / 2), d / 2 - a))[side]
            rows.append(np.stack([cx + u * np.cos(yaw) - v * np.sin(yaw), cy + u * np.sin(yaw) + v * np.cos(yaw), np.full_like(a, h)], -1))
    for k in range(4):
        a = np.arange(0, TOWN_SIDE, 0.5)
        rows.append(np.stack([a, np.full_like(a, 20.0 + 40 * k) + 3 * np.sin(a / 9 + k), np.full_like(a, 2.0 + 0.4 * k)], -1))
    return np.concatenate(rows)


def town_places():
    """41 places at least 10 m apart: a grid of 12 m, headings 0; place 20 is the one the query comes back to."""
    g = np.arange(35.0, 35.0 + 12 * 7, 12.0)
    xy = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)[:41]
    return xy


def seen_from(sv, world, params, x, y, yaw):
    """The descriptor of the town from a pose: the rows within reach, under the world-to-vehicle words of the pose."""
    near = world[(np.abs(world[:, 0] - x) < 1.5 * TOWN_R_MAX) & (np.abs(world[:, 1] - y) < 1.5 * TOWN_R_MAX)]
    cams = sv.voxel_render_cams(sv.voxel_map_pose(np.array([x]), np.array([y]), np.array([yaw])))
    return sv.place_descriptor(near[None].astype(np.float32), None, np.array([len(near)], np.int32), params, cams), len(near)
