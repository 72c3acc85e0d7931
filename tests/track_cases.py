"""Inputs for the object links (group (AB)): a painted 48 x 32 case whose numbers are worked out by hand, random matches against random
boxes, the clamps, and a synthetic scene with one moving box whose motion is known.  The independent model is
stereo_vision.sv.object_links_brute, one Python loop per match."""
import math

import numpy as np

from flow_cases import KITTI, IDENTITY, pose_of, rotation

FIELDS = (("votes", np.int32), ("link", np.int32), ("sums", np.int64))
SMALL = dict(f=40.0, cx=23.5, cy=15.5, q32=2.0, q33=0.0, width=48, height=32, size=1.0, half_px=0.0)  # of the painted 48 x 32 case
ORDER = ("matches", "counts", "poses", "boxes0", "n0", "q0", "boxes1", "n1", "q1")


def same(got, want):
    """Shape, dtype and bits of votes, link and sums."""
    for k, dtype in FIELDS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.dtype != dtype or a.tobytes() != b.tobytes():
            return False
    return True


def call(fn, case, **over):
    """fn(matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1, camera, width, height, words...) of a case dict, words overridden."""
    words = dict(case["words"], **over)
    return fn(*[case[k] for k in ORDER], case["camera"], case["width"], case["height"], **words)


# ------------------------------------------------------------------------------------------------------- the painted 48 x 32 case

# (u0, v0, d0q, u1, v1, d1q).  Previous boxes: P0 = columns [4, 16) x rows [4, 14) at 4 q = 80, P1 = (20, 18, 40, 20) = columns [20, 47) x
# rows [18, 31) - it reaches behind the map, whose last column and row belong to no box - without a depth test.  Current boxes: C0 =
# [5, 17) x [5, 15) at 80, C1 = [8, 20) x [6, 16) without a depth test, over C0; C2 = [22, 42) x [18, 30) at 40.  band_q = 8.
PAINTED_MATCHES = [
    (6, 6, 80, 9, 7, 80),       # 0  P0 -> C0 and C1
    (7, 8, 88, 10, 9, 72),      # 1  both disparities at the band: P0 -> C0 and C1
    (8, 8, 89, 10, 9, 80),      # 2  d0q one beyond the band: in no box
    (15, 13, 80, 16, 14, 80),   # 3  P0's last column and row -> C0's last column and row, and C1
    (16, 10, 80, 12, 10, 80),   # 4  the column behind P0's last: in no box
    (10, 10, 80, 12, 10, -1),   # 5  d1q = -1: P0 -> C1 only (C0 tests the depth), and in no sum
    (10, 11, 0, 12, 10, 80),    # 6  d0q = 0: skipped
    (11, 11, 80, 6, 6, 80),     # 7  P0 -> C0 only: 4 votes each for C0 and C1, the tie goes to C0
    (25, 20, 40, 26, 20, 40),   # 8  P1 -> C2
    (46, 30, 44, 41, 29, 48),   # 9  P1's last column and row -> C2's last column and row, d1q at the band
    (30, 31, 40, 30, 25, 40),   # 10 the map's last row: in no box
    (47, 20, 40, 30, 25, 40),   # 11 the map's last column: in no box
    (30, 25, 200, 30, 25, 47),  # 12 P1 has no depth test -> C2
    (22, 22, 40, 10, 10, 80),   # 13 P1 -> C0 and C1
]
PAINTED_VOTES = [[4, 4, 0, 5], [1, 1, 3, 4], [0, 0, 0, 0]]
PAINTED_LINK = [[0, 4, 5, 4], [2, 3, 4, 1], [-1, 0, 0, 0]]
PAINTED_N = [4, 3, 0]  # of the sums: matches 0, 1, 3, 7 and 8, 9, 12


def painted(skip=()):
    """The painted case, B = 1, capacity 16, max_boxes 3 with 2 previous and 3 current boxes; the row behind n0 holds a box over the whole
    map that must not count.  skip: matches whose d0q is made 0."""
    m = np.full((1, 16, 6), -1, np.int32)
    m[0, :len(PAINTED_MATCHES)] = PAINTED_MATCHES
    for i in skip:
        m[0, i, 2] = 0
    return dict(matches=m, counts=np.array([len(PAINTED_MATCHES)], np.int32), poses=pose_of(np.eye(3), (0.01, 0.0, -0.05))[None].copy(),
                boxes0=np.array([[(4, 4, 12, 10), (20, 18, 40, 20), (0, 0, 48, 32)]], np.int32), n0=np.array([2], np.int32), q0=np.array([[20, 0, 0]], np.int32),
                boxes1=np.array([[(5, 5, 12, 10), (8, 6, 12, 10), (22, 18, 20, 12)]], np.int32), n1=np.array([3], np.int32), q1=np.array([[20, 0, 10]], np.int32),
                camera=dict(SMALL), width=48, height=32, words=dict(band_q=8, min_votes=3, share=128))


def painted_contest(skip):
    """The painted matches against ONE current box over the whole map: both previous boxes vote for it."""
    c = painted(skip)
    c["boxes1"] = np.array([[(0, 0, 48, 32), (0, 0, 0, 0), (0, 0, 0, 0)]], np.int32)
    c["n1"], c["q1"] = np.array([1], np.int32), np.zeros((1, 3), np.int32)
    return c


# ------------------------------------------------------------------------------------------------------- random matches and boxes

def _project(cam, X):
    f, cx, cy, b = cam["f"], cam["cx"], cam["cy"], 1.0 / cam["q32"]
    u = np.floor(f * X[:, 0] / X[:, 2] + cx + 0.5).astype(np.int64)
    v = np.floor(f * X[:, 1] / X[:, 2] + cy + 0.5).astype(np.int64)
    return u, v, np.floor(16.0 * f * b / X[:, 2] + 0.5).astype(np.int64)


def _points(cam, u0, v0, d0q):
    f, cx, cy, b = cam["f"], cam["cx"], cam["cy"], 1.0 / cam["q32"]
    return np.stack([(u0 - cx) * (16.0 * b) / d0q, (v0 - cy) * (16.0 * b) / d0q, f * (16.0 * b) / d0q], 1)


def random_case(seed, n=2000, n0=17, n1=9, M=20, B=2, cam=KITTI):
    """B frames of n matches under a small motion - a fifth outliers, a fifth without d1q, some garbage disparities - against n0 and n1
    random boxes of max_boxes M, some of them without a depth test, some reaching out of the map; frame 1 has its counts the other way
    round and a count above the capacity."""
    rng = np.random.default_rng(7000 + seed)
    W, H = cam["width"], cam["height"]
    matches, poses = np.zeros((B, n, 6), np.int32), np.zeros((B, 12))
    for b in range(B):
        u0, v0 = rng.integers(0, W, n), rng.integers(0, H, n)
        d0q = np.floor(16.0 * rng.uniform(3.0, 60.0, n) + 0.5).astype(np.int64)
        R = rotation(*(math.radians(a) for a in rng.uniform(-0.8, 0.8, 3)))
        t = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1), rng.uniform(-1.5, 0.2)])
        u1, v1, d1q = _project(cam, _points(cam, u0, v0, d0q) @ R.T + t)
        out = rng.random(n) < 0.2
        u1, v1 = np.where(out, u1 + rng.integers(-30, 31, n), u1), np.where(out, v1 + rng.integers(-15, 16, n), v1)
        d1q = np.where(rng.random(n) < 0.2, -1, d1q)
        d0q[::97] = (0, -5, 2 ** 20 + 1, 2 ** 31 - 1)[seed % 4]
        matches[b], poses[b] = np.stack([u0, v0, d0q, u1, v1, d1q], 1), pose_of(R, t + rng.uniform(-0.02, 0.02, 3))

    def boxes():
        x, y = rng.integers(-40, W - 20, (B, M)), rng.integers(-30, H - 20, (B, M))
        w, h = rng.integers(30, 500, (B, M)), rng.integers(20, 250, (B, M))
        q = np.where(rng.random((B, M)) < 0.3, rng.integers(-2, 1, (B, M)), rng.integers(12, 240, (B, M)))
        return np.stack([x, y, w, h], 2).astype(np.int32), q.astype(np.int32)

    (boxes0, q0), (boxes1, q1) = boxes(), boxes()
    counts = np.array([n - 3] + [n + 5] * (B - 1), np.int32)
    return dict(matches=matches, counts=counts, poses=poses, boxes0=boxes0, n0=np.array([n0] + [n1] * (B - 1), np.int32), q0=q0, boxes1=boxes1,
                n1=np.array([n1] + [n0] * (B - 1), np.int32), q1=q1, camera=dict(cam), width=W, height=H,
                words=dict(band_q=(64, 160, 2 ** 20, 96)[seed % 4], min_votes=(1, 2, 3, 5)[seed % 4], share=(0, 64, 128, 32)[seed % 4]))


# ------------------------------------------------------------------------------------------------------- the clamps

def clamp_case(pose=None):
    """Four matches with d1q = 1 under a camera with a baseline of 10 km, in one box over the map: X1 is some 1e8 m from Xc on every axis,
    so m sits at +-2^20 and p at +-2^30.  Targets left and right of cx, above cy: x takes both signs, y is negative, z positive."""
    cam = dict(KITTI, q32=1e-4)
    m = np.array([[(600, 170, 2 ** 20, 10, 3, 1), (620, 180, 2 ** 20, 1200, 5, 1), (640, 190, 2 ** 20, 20, 2, 1), (300, 100, 2 ** 20, 30, 1, 1)]], np.int32)
    box = np.array([[(0, 0, 5000, 5000)]], np.int32)
    return dict(matches=m, counts=np.array([4], np.int32), poses=(pose_of(np.eye(3), (5000.0, -5000.0, 300.0)) if pose is None else np.asarray(pose, np.float64))[None].copy(),
                boxes0=box, n0=None, q0=np.zeros((1, 1), np.int32), boxes1=box.copy(), n1=None, q1=np.zeros((1, 1), np.int32), camera=cam, width=1242, height=375,
                words=dict(band_q=0, min_votes=1, share=256))


# ------------------------------------------------------------------------------------------------------- a scene with a known answer

MOVING_TRUTH = (0.30, -0.04, 0.50)  # metres per frame, in the current camera's axes
MOVING_GATE_M = 256                 # 1/1024 m: the gated round keeps what lies within 0.25 m of the first round's mean


def moving_scene(seed, cam=KITTI):
    """600 static points (disparities of 6 to 40 px) and a box of 120 points at some 16 m that moves by MOVING_TRUTH between the frames,
    under a camera that drives 1.1 m forward and turns a little; whole-pixel targets, d1 to 1/16 px, 15 % outliers on both.  Box 0 is the
    moving box and tests the depth, box 1 a static box without a depth test.  -> the case (its poses the identity: the test fits them)."""
    rng = np.random.default_rng(9000 + seed)
    W, H = cam["width"], cam["height"]
    R = rotation(math.radians(0.2), math.radians(-0.6), math.radians(0.1))
    t = np.array([0.02, -0.01, -1.10])
    u0 = np.concatenate([rng.integers(0, W, 600), rng.integers(700, 820, 120)])
    v0 = np.concatenate([rng.integers(0, H, 600), rng.integers(150, 230, 120)])
    d0q = np.floor(16.0 * np.concatenate([rng.uniform(6.0, 40.0, 600), rng.uniform(23.5, 24.5, 120)]) + 0.5).astype(np.int64)
    Xc = _points(cam, u0, v0, d0q) @ R.T + t
    Xc[600:] += np.asarray(MOVING_TRUTH)
    u1, v1, d1q = _project(cam, Xc)
    out = rng.random(720) < 0.15
    u1, v1 = np.where(out, u1 + rng.integers(-30, 31, 720), u1), np.where(out, v1 + rng.integers(-15, 16, 720), v1)
    order = rng.permutation(720)
    m = np.stack([u0, v0, d0q, u1, v1, d1q], 1)[order].astype(np.int32)[None].copy()
    boxes0 = np.array([[(700, 150, 120, 80), (100, 80, 300, 220)]], np.int32)
    boxes1 = np.array([[(690, 140, 180, 120), (60, 50, 380, 300)]], np.int32)
    q = np.array([[96, 0]], np.int32)  # 24 px in quarter pixels
    return dict(matches=m, counts=np.array([720], np.int32), poses=IDENTITY[None].copy(), boxes0=boxes0, n0=None, q0=q, boxes1=boxes1, n1=None, q1=q.copy(),
                camera=dict(cam), width=W, height=H, words=dict(band_q=48, min_votes=3, share=128))
