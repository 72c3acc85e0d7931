"""The graphs tests/test_pose_graph.py runs: the shapes at which the kernels of group (AE) can go wrong, the small graphs of the dense
check, and the drive of DESIGN.md §4ad extended to three passes of the street.  Plain numpy; the data are made with matrix products,
the definitions under test are not used to make them."""
import numpy as np

import voxel_repose_cases as repose

LAM = 1e-6


def rot(om):
    """Rodrigues: [n,3] -> [n,3,3]."""
    om = np.asarray(om, np.float64).reshape(-1, 3)
    angle = np.sqrt((om * om).sum(1))
    K = np.zeros((len(om), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -om[:, 2], om[:, 1], om[:, 2], -om[:, 0], -om[:, 1], om[:, 0]
    small = angle < 1e-8
    a = np.where(small, 1.0, angle)
    s, c = np.where(small, 1.0, np.sin(a) / a), np.where(small, 0.5, (1.0 - np.cos(a)) / (a * a))
    return np.eye(3)[None] + s[:, None, None] * K + c[:, None, None] * (K @ K)


def pack(R, t):
    return np.ascontiguousarray(np.concatenate([R.reshape(-1, 9), t.reshape(-1, 3)], 1))


def unpack(P):
    return P[:, :9].reshape(-1, 3, 3), P[:, 9:]


def between(Pa, Pb):
    """Pa^-1 o Pb, row by row."""
    Ra, ta = unpack(Pa)
    Rb, tb = unpack(Pb)
    Rt = Ra.transpose(0, 2, 1)
    return pack(Rt @ Rb, (Rt @ (tb - ta)[:, :, None])[:, :, 0])


def nudged(P, rng, s_rot, s_trans, keep=None):
    """P o (a small random motion), row by row; the rows of `keep` stay."""
    R, t = unpack(P)
    n = len(P)
    out = pack(R @ rot(rng.normal(0.0, s_rot, (n, 3))), t + (R @ rng.normal(0.0, s_trans, (n, 3, 1)))[:, :, 0])
    if keep is not None:
        out[keep] = P[keep]
    return out


def path(N, rng):
    """N poses along a winding path: about a metre a frame, rotations about all three axes."""
    k = np.arange(N, dtype=np.float64)
    R = rot(np.stack([0.1 * np.sin(k / 50.0), 0.1 * np.cos(k / 70.0), 0.02 * k + 0.3 * np.sin(k / 9.0)], 1))
    t = np.cumsum(rng.normal(0.0, 0.6, (N, 3)) + np.array([0.8, 0.0, 0.0]), 0)
    return pack(R, t)


def graph(N, extra, seed, fixed=(0,), chain=True, noise=(0.01, 0.05)):
    """A case: the chain 0 - 1 - ... - N - 1 (where asked) and the edges `extra` = [(i, j), ...] over a winding path; the measurements are
    the truth's, nudged, so the loops are inconsistent; the poses start away from the truth; the weights are spread over two decades."""
    rng = np.random.default_rng(seed)
    truth = path(N, rng)
    mask = np.zeros(N, bool)
    mask[list(fixed)] = True
    e = ([(k, k + 1) for k in range(N - 1)] if chain else []) + list(extra)
    i, j = (np.array([p[c] for p in e], np.int32).reshape(-1) for c in (0, 1))
    Z = nudged(between(truth[i], truth[j]), rng, *noise) if len(e) else np.zeros((0, 12))
    w = np.ascontiguousarray(10.0 ** rng.uniform(-0.3, 2.3, (len(e), 2)))
    return dict(poses=nudged(truth, rng, 0.03, 0.3, keep=mask), fixed=mask, i=i, j=j, Z=Z, w=w, lam=LAM, truth=truth)


def shape_cases():
    """{name: case}: shared by the CPU tests (the numpy form against the plain loops) and the GPU tests (the device against the numpy
    form).  A case: poses, fixed, i, j, Z, w, lam - and iters, the iteration counts the solver is run for."""
    out = {}
    out["one_pose_no_edge"] = graph(1, [], 1, fixed=(0,))
    out["one_free_pose_no_edge"] = graph(1, [], 2, fixed=())
    out["one_edge"] = graph(2, [], 3)
    out["triangle"] = graph(3, [(2, 0)], 4)
    for N in (255, 256, 257):  # the edge of a chunk: one chunk full but one lane, full, and one pose in the second
        out["chain_%d" % N] = graph(N, [(0, N - 1), (N // 2, 3)], N)
    hub = [(7, k) for k in range(20, 170)] + [(k, 7) for k in range(170, 320)]
    out["hub_of_300"] = graph(400, hub, 5)
    out["backwards_and_twice"] = graph(40, [(30, 2), (30, 2), (2, 30), (39, 0), (17, 16), (16, 17)], 6)
    g = graph(60, [(50, 5), (10, 40), (59, 0), (20, 21)], 7)
    g["w"][5] = 0.0          # an odometry edge switched off
    g["w"][60] = 0.0         # a loop switched off
    g["w"][8, 0] = 0.0       # rotation unweighted only
    g["w"][9, 1] = 0.0       # translation unweighted only
    g["w"][29:31] = 0.0      # pose 30 is left without a live edge: lam alone holds it
    out["zero_weights_and_a_lonely_pose"] = g
    out["no_chain"] = graph(50, [(0, 10), (10, 20), (20, 0), (30, 31)], 8, chain=False)  # poses without any entry in the lists
    out["fixed_in_the_middle"] = graph(70, [(60, 3)], 9, fixed=(33,))
    out["fixed_at_both_ends"] = graph(70, [(60, 3)], 10, fixed=(0, 69))
    out["all_fixed"] = graph(20, [(15, 3)], 11, fixed=tuple(range(20)))
    for g in out.values():
        g["iters"] = (1, 2, 3, 17)
    rng = np.random.default_rng(12)
    N = 65537  # 257 chunks: the third level of the tree
    far = rng.integers(0, N, (600, 2))
    far = far[far[:, 0] != far[:, 1]]
    out["third_level"] = dict(graph(N, [tuple(p) for p in far.tolist()], 12), iters=(3,))
    return out


def dense_cases():
    """The small graphs (at most 20 poses) of the dense check: loops that contradict one another, so that the least cost is far from zero."""
    far = dict(noise=(0.05, 0.5))  # measurements 50 mrad and half a metre off one another
    return {"triangle": graph(3, [(2, 0)], 21, **far), "ring_of_8": graph(8, [(7, 0), (5, 1), (1, 5)], 22, **far),
            "web_of_20": graph(20, [(19, 0), (15, 3), (3, 15), (10, 2), (18, 7)], 23, **far), "held_in_the_middle": graph(12, [(11, 0), (9, 2)], 24, fixed=(6,), **far)}


def consistent_case():
    """Exact relative motions, a drifted start, pose 0 fixed: the least cost is zero and lies at the truth."""
    rng = np.random.default_rng(31)
    N = 20
    truth = path(N, rng)
    e = [(k, k + 1) for k in range(N - 1)] + [(19, 0), (15, 3), (3, 12), (10, 2)]
    i, j = (np.array([p[c] for p in e], np.int32) for c in (0, 1))
    mask = np.zeros(N, bool)
    mask[0] = True
    return dict(poses=nudged(truth, rng, 0.02, 0.2, keep=mask), fixed=mask, i=i, j=j, Z=between(truth[i], truth[j]), w=np.ascontiguousarray(10.0 ** rng.uniform(0.0, 2.0, (len(e), 2))),
                lam=LAM, truth=truth)


# ------------------------------------------------------------------------------------------------------------------ the drive

PASSES = ((0, 40), (60, 100), (120, 160))  # the frames of the three passes of the street; between them the vehicle backs out of it
FRAMES = 160
KEYS = (5, 15, 25, 35)                     # the keyframes of the first pass that the later passes find again: a loop is a run of matches
LOOP_EDGES = tuple((k, 60 + k) for k in KEYS) + tuple((k, 120 + k) for k in KEYS)  # both later passes close onto the first
SPREAD_EDGES = ((25, 85), (25, 145))       # what loop_spread can take of them: one edge a loop; the two loops share the frames 25 .. 85
FALSE_LOOP = (35, 110)                     # a wrong place match: frame 110 is 16 m down the street, backing out
XI = np.array([0.0, 0.0, 0.02, 0.3, 2.0, 0.1])  # §4ad's drift, spread over the drive
W_ODOMETRY = (2.5e7, 2500.0)  # sigma = 0.2 mrad and 2 cm a frame: this odometry turns far better than it measures its way
W_LOOP = (2.5e5, 2500.0)      # sigma = 2 mrad and 2 cm: the noise of the loop measurements below
GATE = 2500.0 * 5.0 ** 2                  # a loop edge that contradicts the odometry by more than 5 m (or 0.5 rad) is no drift of this drive


def drive_truth(sv):
    """The true poses [160,12]: §4ad's pass along x three times, each 0.37 m further along and 0.2 m further to the side.  Between the
    passes the vehicle backs out of the street, 2 m a frame on a lane of its own, heading as before: §4ad's way round the block - 40 m
    and a half-turn in one step - puts a metre of error on single odometry edges, and a half-turn mirrors a drift that is fixed in the
    vehicle's axes, as the spread model's is, which no relative motion reveals."""
    k = np.arange(FRAMES)
    x, y, yaw = np.zeros(FRAMES), np.zeros(FRAMES), np.zeros(FRAMES)
    for n, (a, b) in enumerate(PASSES):
        x[a:b], y[a:b], yaw[a:b] = np.arange(b - a) + 0.37 * n, 0.2 * n, 0.01 * np.sin(k[a:b])
    for n, (a, b) in enumerate(((40, 60), (100, 120))):
        x[a:b], y[a:b] = 39.0 - (k[a:b] - a) * 2.0, 0.2 * n + 0.1
    return sv.voxel_map_pose(x, y, yaw)


def drive_frames(sv, truth):
    """repose.drive_frames for the three passes: per frame the surface points 2 .. 5 m ahead, none while the block is driven round."""
    W = repose.drive_surfaces()
    rows = []
    for k in range(FRAMES):
        if not any(a <= k < b for a, b in PASSES):
            rows.append(np.zeros((0, 3)))
            continue
        inv = sv._pose_inv(truth[k])
        Pf = W @ inv[:9].reshape(3, 3).T + inv[9:]
        rows.append(Pf[(Pf[:, 0] >= 2.0) & (Pf[:, 0] <= 5.0)])
    cap = max(len(r) for r in rows)
    xyz = np.zeros((FRAMES, cap, 3))
    for k, r in enumerate(rows):
        xyz[k, :len(r)] = r
    return xyz, None, None, np.array([len(r) for r in rows], np.int32)


def drive(sv):
    """-> truth, the drifted poses, the loop measurements {(i, j): Z} - the truth's with 2 mrad and 2 cm of noise -, the false one (i, j, Z)."""
    truth = drive_truth(sv)
    drift = np.array([sv._pose_mul(truth[k], sv.pose_exp(-(k / (FRAMES - 1)) * XI)) for k in range(FRAMES)])
    rng = np.random.default_rng(41)
    loops = {(i, j): nudged(between(truth[i:i + 1], truth[j:j + 1]), rng, 0.002, 0.02)[0] for i, j in LOOP_EDGES}
    false = FALSE_LOOP + (nudged(between(truth[:1], truth[:1]), rng, 0.002, 0.02)[0],)  # "the two frames stand at one place"
    return truth, drift, loops, false


def drive_graph(sv, drift, loops, false):
    edges = [sv.pose_graph_chain(drift, *W_ODOMETRY)] + [sv.pose_graph_loop(i, j, Z, *W_LOOP) for (i, j), Z in loops.items()] + [sv.pose_graph_loop(false[0], false[1], false[2], *W_LOOP)]
    return sv.pose_graph(drift, edges, fixed=(0,))


def drive_spread(sv, drift, loops):
    """The baseline the repository had: loop_spread on one edge of each loop, one loop after the other."""
    out = drift
    for i, j in SPREAD_EDGES:
        out = sv.loop_spread(out, i, j, sv._pose_mul(out[i], loops[(i, j)]))
    return out


def seen():
    """The frames that see the street: those of the three passes."""
    return np.concatenate([np.arange(a, b) for a, b in PASSES])
