"""Inputs for the stereo visual odometry (group (Z)): painted image pairs for the temporal matcher, random matches for the sums of a pose
round and synthetic scenes with a known motion for the egomotion loop.  The independent model of the sums is
stereo_vision.sv.flow_pose_sums_brute, one Python loop per match."""
import math

import numpy as np

KITTI = dict(f=721.54, cx=609.56, cy=172.85, q32=1.0 / 0.537, q33=0.0, width=1242, height=375, size=1.0, half_px=0.0)  # voxel_render_camera's words
SMALL = dict(f=40.0, cx=15.5, cy=11.5, q32=2.0, q33=0.0, width=32, height=24, size=1.0, half_px=0.0)  # of the painted 24 x 32 pair
IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
_MATRIX = "%s: !!opencv-matrix\n   rows: %d\n   cols: %d\n   dt: d\n   data: [ %s ]\n"
_K = "721.54, 0.0, 609.56, 0.0, 721.54, 172.85, 0.0, 0.0, 1.0"
# The committed KITTI frames are rectified already: their rig is two equal pinhole cameras 0.537 m apart, not the raw cameras of the
# package's default calibration file.
RECTIFIED_YML = ("%YAML:1.0\n" + _MATRIX % ("K1", 3, 3, _K) + _MATRIX % ("K2", 3, 3, _K) + _MATRIX % ("D1", 1, 5, "0.0, 0.0, 0.0, 0.0, 0.0")
                 + _MATRIX % ("D2", 1, 5, "0.0, 0.0, 0.0, 0.0, 0.0") + _MATRIX % ("R", 3, 3, "1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0") + "T: [ -0.537, 0.0, 0.0 ]\n")
FIELDS = ("matches", "cost", "counts")


def same(got, want, fields=FIELDS):
    """Shape, dtype (int32) and bits of every field."""
    for k in fields:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.dtype != np.int32 or a.tobytes() != b.tobytes():
            return False
    return True


def rotation(rx, ry, rz):
    """R = Rz Ry Rx of angles in radians."""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose_of(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def angle_between(Ra, Rb):
    """The angle of Ra Rb^T in degrees."""
    D = np.asarray(Ra).reshape(3, 3) @ np.asarray(Rb).reshape(3, 3).T
    axis = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return math.degrees(math.atan2(0.5 * math.sqrt(float((axis * axis).sum())), 0.5 * (np.trace(D) - 1.0)))


# ------------------------------------------------------------------------------------------------------- the painted 24 x 32 pair

def texture(seed, H, W, smooth=0):
    """A random uint8 image; smooth > 0 averages it over (2 smooth + 1)^2 boxes, so that neighbouring candidates cost nearly the same."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H + 2 * smooth, W + 2 * smooth)).astype(np.float64)
    if smooth:
        k = 2 * smooth + 1
        v = np.lib.stride_tricks.sliding_window_view(img, (k, k))
        img = v.mean((2, 3))
    return np.ascontiguousarray(img[:H, :W].astype(np.uint8))


def painted():
    """prev, cur uint8 [1,24,32] and d_prev, d_cur float32 [1,24,32] for PAINTED_WORDS (step 4, r 2, wx = wy = 2).  Both images are flat 100
    but for what is painted; d_prev is 8 px at the painted lattice points and invalid (-1) elsewhere, d_cur 4 px.  A bright pixel (200) at
    the point in prev and one at the point + flow in cur gives a best of 0 there; a candidate whose patch misses cur's pixel costs 100, one
    that holds it elsewhere 200.
      A (4, 4)    the first admissible row and column; flow (+1, +1); the candidates at centre column or row 2 miss the pixel: second 100.
      F (12, 4)   flat: 0 against 0, no match.
      T (20, 4)   cur bright at (19, 4) and (20, 4): the candidates (-1, 0) and (0, 0) both cost 100 - the other pixel -, the tie goes to
                  (-1, 0), the lower index; (0, 0) is its neighbour, so the second is 200: (+2, 0), which holds (20, 4) alone.
      U (8, 12)   flow (+1, +1), second 100.
      R (20, 12)  cur bright at (22, 12): the best, 0, is on the window's rim - no match.
      S (28, 12)  vertical stripes of period 2 in both images over columns 25 .. 31, rows 9 .. 15: (0, -1), (0, 0) and (0, +1) cost 0, the
                  best is (0, -1) and (0, +1), two away, is the second: the ratio test rejects 0 against 0.
      D (8, 20)   flow (-1, 0), second 100 ((+2, 0) misses the pixel); the test makes d_prev there 0, negative, inf and NaN in turn.
      C (16, 20)  flow (0, -1); every candidate holds cur's pixel: second 200; d_cur at the target (16, 19) is NaN: d1q = -1.
      L (28, 20)  the last admissible row and column; flow (-1, -1); the candidates at centre column 30 and row 22 would leave the image;
                  all others hold the pixel: second 200."""
    prev = np.full((24, 32), 100, np.uint8)
    cur = np.full((24, 32), 100, np.uint8)
    d_prev = np.full((24, 32), -1.0, np.float32)
    d_cur = np.full((24, 32), 4.0, np.float32)
    for (u, v), targets in (((4, 4), [(5, 5)]), ((12, 4), []), ((20, 4), [(19, 4), (20, 4)]), ((8, 12), [(9, 13)]), ((20, 12), [(22, 12)]), ((28, 12), []),
                            ((8, 20), [(7, 20)]), ((16, 20), [(16, 19)]), ((28, 20), [(27, 19)])):
        d_prev[v, u] = 8.0
        if targets:
            prev[v, u] = 200
        for tu, tv in targets:
            cur[tv, tu] = 200
    for v in range(9, 16):
        for u in range(25, 32):
            prev[v, u] = cur[v, u] = 60 + 120 * (u % 2)
    d_cur[19, 16] = np.nan
    return prev[None], cur[None], d_prev[None], d_cur[None]


PAINTED_WORDS = dict(step=4, r=2, wx=2, wy=2, ratio=230, capacity=16)
PAINTED_D = (8, 20)  # the point whose d_prev the test spoils
# (u0, v0, d0q, u1, v1, d1q), (best, second) in point order: ascending v0 * W + u0
PAINTED_WANT = [((4, 4, 128, 5, 5, 64), (0, 100)), ((20, 4, 128, 19, 4, 64), (100, 200)), ((8, 12, 128, 9, 13, 64), (0, 100)), ((8, 20, 128, 7, 20, 64), (0, 100)),
                ((16, 20, 128, 16, 19, -1), (0, 200)), ((28, 20, 128, 27, 19, 64), (0, 200))]


def shifted_halves(seed=5, H=48, W=96, smooth=0):
    """A random texture whose left half moves by (+3, -2) and whose right half by (-5, +1) from prev to cur: cur[v, u] = prev[v - dy, u -
    dx] inside a half; the pixels a shift uncovers are fresh noise.  -> prev, cur [1,H,W], d_prev, d_cur float32 [1,H,W] (random, some
    invalid), the flows ((3, -2), (-5, 1)) and the column where the halves meet."""
    rng = np.random.default_rng(seed)
    prev = texture(seed, H, W, smooth)
    cur = rng.integers(0, 256, (H, W)).astype(np.uint8)
    half = W // 2
    flows = ((3, -2), (-5, 1))
    for (dx, dy), (x0, x1) in zip(flows, ((0, half), (half, W))):
        for v in range(H):
            for u in range(x0, x1):
                su, sv_ = u - dx, v - dy
                if x0 <= su < x1 and 0 <= sv_ < H:
                    cur[v, u] = prev[sv_, su]
    d_prev = rng.uniform(1.0, 60.0, (H, W)).astype(np.float32)
    d_cur = rng.uniform(1.0, 60.0, (H, W)).astype(np.float32)
    d_prev[rng.random((H, W)) < 0.1] = -1.0
    d_cur[rng.random((H, W)) < 0.2] = -1.0
    return prev[None], cur[None], d_prev[None], d_cur[None], flows, half


# ------------------------------------------------------------------------------------------------------- matches for the sums

def scene(seed, n=1500, rot_deg=(0.4, -1.0, 0.2), t=(0.02, -0.01, -1.17), outliers=0.2, no_d1=0.3, cam=KITTI):
    """The synthetic egomotion case: n matches of points with disparities of 3 to 60 px under the motion (R, t), u1 and v1 rounded to whole
    pixels, d1 to 1/16 px; a share of outliers moved by up to +-30 x +-15 px, a share without d1.  -> (matches int32 [1,n,6], counts int32
    [1], the true pose [12])."""
    rng = np.random.default_rng(seed)
    f, cx, cy, b = cam["f"], cam["cx"], cam["cy"], 1.0 / cam["q32"]
    u0 = rng.integers(0, cam["width"], n)
    v0 = rng.integers(0, cam["height"], n)
    d0q = np.floor(16.0 * rng.uniform(3.0, 60.0, n) + 0.5).astype(np.int64)
    X0 = np.stack([(u0 - cx) * (16.0 * b) / d0q, (v0 - cy) * (16.0 * b) / d0q, f * (16.0 * b) / d0q], 1)
    R = rotation(*(math.radians(a) for a in rot_deg))
    Xc = X0 @ R.T + np.asarray(t)
    u1 = np.floor(f * Xc[:, 0] / Xc[:, 2] + cx + 0.5).astype(np.int64)
    v1 = np.floor(f * Xc[:, 1] / Xc[:, 2] + cy + 0.5).astype(np.int64)
    d1q = np.floor(16.0 * f * b / Xc[:, 2] + 0.5).astype(np.int64)
    out = rng.random(n) < outliers
    u1 = np.where(out, u1 + rng.integers(-30, 31, n), u1)
    v1 = np.where(out, v1 + rng.integers(-15, 16, n), v1)
    d1q = np.where(rng.random(n) < no_d1, -1, d1q)
    m = np.stack([u0, v0, d0q, u1, v1, d1q], 1).astype(np.int32)
    return m[None].copy(), np.array([n], np.int32), pose_of(R, t)


SCENE_SCALES = (1.0, 0.6, 0.3, 0.0)  # of the rotation (0.4, -1.0, 0.2) degrees, by seed


def scene_of(seed, n=1500):
    s = SCENE_SCALES[seed % 4]
    return scene(100 + seed, n, rot_deg=(0.4 * s, -1.0 * s, 0.2 * s))


def random_sums_case(seed):
    """(matches [3,cap,6], counts [3], camera, poses [3,12], gate_q, dgate_q) for flow_pose_sums against the brute model: frame 0 a scene
    with outliers, frame 1 a count of 0 or -1, frame 2 a scene with points behind the camera, garbage rows and a count above the
    capacity.  Variants by seed: exact and float32-rounded disparities, with and without d1, gates of 0, tight and none, a pose that is
    not finite."""
    rng = np.random.default_rng(1000 + seed)
    cap = int(rng.integers(20, 90))
    cam = dict(KITTI) if seed % 2 else dict(KITTI, f=float(np.float32(718.856)), cx=607.1928, cy=185.2157, q32=float(1.0 / np.float32(0.54)))
    m0, _, pose = scene(seed, cap, rot_deg=tuple(rng.uniform(-1.5, 1.5, 3)), t=tuple(rng.uniform(-0.5, 0.5, 2)) + (float(rng.uniform(-1.5, 0.5)),),
                        no_d1=(0.0, 0.3, 1.0)[seed % 3])
    m2, _, pose2 = scene(seed + 50, cap, t=(0.0, 0.0, float(rng.uniform(-12.0, -6.0))))  # disparities of up to 60 px: from 6.5 m on - the near points end up behind
    if seed % 4 == 1:  # disparities as a float32 map holds them: any sixteenth
        m0[0, :, 2] = np.floor(16.0 * np.float32(m0[0, :, 2] / 16.0 + rng.uniform(-0.03, 0.03, cap)).astype(np.float64) + 0.5)
    m2[0, ::7, 2] = (0, -5, 2 ** 20 + 1, 2 ** 31 - 1)[seed % 4]  # garbage disparities: skipped
    m2[0, 3::11, 3] = (2 ** 31 - 1, -2 ** 31)[seed % 2]           # garbage targets: no inliers, and no overflow
    matches = np.concatenate([m0, np.zeros_like(m0), m2]).astype(np.int32)
    counts = np.array([cap - seed % 3, (0, -1)[seed % 2], cap + 5], np.int32)
    poses = np.stack([pose, IDENTITY, pose2])
    if seed % 5 == 0:
        poses[0, seed % 12] = (np.nan, np.inf)[seed % 2]
    gate = (None, 0, 16, 48, 320)[seed % 5]
    dgate = (None, 0, 8, 32)[seed % 4]
    return matches, counts, cam, poses, gate, dgate
