"""Inputs for the temporal warp of disparity maps (group (AA)): painted 24 x 32 maps under flow_cases.SMALL with the numbers they must
give worked out by hand, random maps, and the shapes of the GPU tests.  The independent model is stereo_vision.sv.disparity_warp_brute,
one Python loop per pixel.

The camera SMALL has f = 40, cx = 15.5, cy = 11.5 and a baseline of 0.5 m: b16 = 8, fb = 20, fb16 = 320.  A pixel (u, v) with a disparity
of d px (d0q = 16 d) stands at z0 = 320 / d0q = 20 / d metres, x0 = (u - 15.5) / (2 d), y0 = (v - 11.5) / (2 d).
  sideways   a translation t = (0.5, 0, 0) leaves z and so pd = d0q, and moves the pixel by 40 * 0.5 / z0 = d columns to the right.
  forward    a translation t = (0, 0, tz) with z = z0 + tz = z0 / s scales the image about (15.5, 11.5) by s and the disparity by s: tu =
             floor(s (u - 15.5) + 16), tv = floor(s (v - 11.5) + 12), pd = s d0q, e = ceil(s) - 1 for a whole d0q.  With d = 8 px (z0 = 2.5):
             tz = -1.25 gives s = 2, tu = 2 u - 15, tv = 2 v - 11, pd = 256, e = 1; tz = -0.5 gives s = 1.25, tu = floor(1.25 u - 3.375), pd = 160, e = 1."""
import numpy as np

from flow_cases import IDENTITY, SMALL, pose_of

H, W = 24, 32
FIELDS = ("expected", "source", "label", "out", "counts")
DTYPES = dict(expected=np.int32, source=np.int32, label=np.uint8, out=np.float32, counts=np.int32)
NONE_BITS = 0xBF800000  # -1.0f


def same(got, want, fields=FIELDS):
    """Shape, dtype and bits of every field; a field the definition leaves None must be None."""
    for k in fields:
        if want[k] is None or got[k] is None:
            if want[k] is not got[k]:
                return False
            continue
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.dtype != DTYPES[k] or a.tobytes() != b.tobytes():
            return False
    return True


def differences(got, want, fields=FIELDS):
    """What same() found, for a failing assertion's message."""
    out = []
    for k in fields:
        if want[k] is None or got[k] is None:
            out.append("%s: %s" % (k, "both None" if want[k] is got[k] else "one is None"))
            continue
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype:
            out.append("%s: %s %s against %s %s" % (k, a.dtype, a.shape, b.dtype, b.shape))
        else:
            bytes_of = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(x.size, -1)
            bad = np.flatnonzero((bytes_of(a) != bytes_of(b)).any(1))
            out.append("%s: %d of %d differ%s" % (k, bad.size, a.size, "" if not bad.size else ", first at %d: %r against %r" % (bad[0], a.ravel()[bad[0]], b.ravel()[bad[0]])))
    return "; ".join(out)


def translate(tx=0.0, ty=0.0, tz=0.0):
    return pose_of(np.eye(3), (tx, ty, tz))


def blank(value=-1.0):
    return np.full((H, W), value, np.float32)


def noise(seed, lo=1.0, hi=20.0, invalid=0.15, shape=(H, W)):
    """A random float32 map, a share of it invalid (-1)."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(lo, hi, shape).astype(np.float32)
    d[rng.random(shape) < invalid] = -1.0
    return d


def _case(name, d_prev, pose, want, kept, covered, d_cur=None, **words):
    """want: {(v, u): (expected, source)} of the pixels a source reaches, every other pixel 0 and -1; None: the test has its own."""
    return dict(name=name, d_prev=d_prev, d_cur=noise(len(name)) if d_cur is None else d_cur, pose=np.asarray(pose, np.float64), want=want, kept=kept, covered=covered, words=words)


def painted():
    """The painted 24 x 32 frames: a list of dicts (name, d_prev, d_cur, pose, words, and by hand want, kept, covered)."""
    cases = []
    src = lambda u, v: v * W + u
    # sideways by d columns: row 5 holds 20 sources u = 0 .. 19 with d = 20 - u px, which all land in column 20 - the nearest, u = 0 with
    # pd = 320, wins; row 7 holds two, u = 3 with 4 px and u = 5 with 2 px, both landing in column 7: the nearer, 64 against 32, wins
    d = blank()
    for u in range(20):
        d[5, u] = 20.0 - u
    d[7, 3], d[7, 5] = 4.0, 2.0
    cases.append(_case("pile_up", d, translate(tx=0.5), {(5, 20): (320, src(0, 5)), (7, 7): (64, src(3, 7))}, 22, 22))
    # forward by s = 1.25: (15, 10) and (16, 10), both 8 px, go to columns 15 and 16 of row floor(1.25 * -1.5 + 12) = 10 with pd = 160 and a
    # cover of 2 x 2: column 16 is reached by both with equal pd - the lower index wins
    d = blank()
    d[10, 15] = d[10, 16] = 8.0
    want = {(v, u): (160, src(15, 10)) for v in (10, 11) for u in (15, 16)}
    want.update({(v, 17): (160, src(16, 10)) for v in (10, 11)})
    cases.append(_case("tie", d, translate(tz=-0.5), want, 2, 8))
    # forward by s = 2: (22, 16) goes to (29, 21) with its whole 2 x 2 cover; (23, 17) to (31, 23), the last column and row, where three
    # of its four pixels are clipped; (7, 5) to (-1, -1), left of column 0 and above row 0, where only (0, 0) is inside; (2, 3) to
    # (-11, -5): kept, and nothing covered
    d = blank()
    d[16, 22] = d[17, 23] = d[5, 7] = d[3, 2] = 8.0
    want = {(v, u): (256, src(22, 16)) for v in (21, 22) for u in (29, 30)}
    want[(23, 31)] = (256, src(23, 17))
    want[(0, 0)] = (256, src(7, 5))
    cases.append(_case("forward_clipped", d, translate(tz=-1.25), want, 4, 6))
    # the cap: (15, 11) with 2 px stands at 10 m; 9 m forward put it at 1 m: s = 10, pd = 320, tu = floor(-5 + 16) = 11, tv = floor(-5 + 12)
    # = 7, and e = 9 before the cap
    d = blank()
    d[11, 15] = 2.0
    for e_max in (0, 1, 4):
        want = {(7 + dy, 11 + dx): (320, src(15, 11)) for dy in range(e_max + 1) for dx in range(e_max + 1)}
        cases.append(_case("cap_%d" % e_max, d, translate(tz=-9.0), want, 1, (e_max + 1) ** 2, e_max=e_max))
    # too near and behind: 8 px stands at 2.5 m; at z = 0.05, 0 and -2.5 nothing is kept
    for k, tz in enumerate((-2.45, -2.5, -5.0)):
        cases.append(_case("near_%d" % k, blank(8.0), translate(tz=tz), {}, 0, 0))
    # a pose word that is not finite: nothing is kept, whatever the word
    for k, (at, bad) in enumerate(((4, np.nan), (9, np.inf), (2, -np.inf), (11, np.nan))):
        pose = IDENTITY.copy()
        pose[at] = bad
        cases.append(_case("pose_%d" % k, noise(40 + k), pose, {}, 0, 0))
    # d_prev that makes no source: 0, negative, inf, NaN, 1e-3 (16 d + 0.5 < 1) and 70000 (beyond 2^20 sixteenths); one that does
    d = blank(0.0)
    d[2, 3], d[2, 4], d[2, 5], d[2, 6], d[2, 7], d[9, 9] = -3.0, np.inf, np.nan, 1e-3, 70000.0, 8.0
    cases.append(_case("bad_d_prev", d, IDENTITY, {(9, 9): (128, src(9, 9))}, 1, 1))
    return cases


def identity_case():
    """d_cur = d_prev under the identity: expected = d0q, source = the pixel itself, every label 3 (or 0)."""
    d = noise(7, 1.0, 60.0)
    d[0, 0], d[H - 1, W - 1] = 60.0, 1.0 / 16
    return d


def threshold_case(rel_q):
    """Under the identity with d_prev = 8 px everywhere (ex = 128): t = 16 + ((rel_q * 128) >> 8), and d_cur at ex +- t and ex +- (t + 1) in
    row 0 -> (d_cur, t, the labels of (0, 0 .. 3): agree, nearer, agree, farther)."""
    t = 16 + ((rel_q * 128) >> 8)
    d_cur = blank(8.0)
    for u, mq in enumerate((128 + t, 128 + t + 1, 128 - t, 128 - t - 1)):
        d_cur[0, u] = mq / 16.0
    return d_cur, t, (3, 4, 3, 5)


def modes_case():
    """One frame with all six labels under the identity (tol_q 16) -> d_prev, d_cur and per pixel of row 0 its label: (0, 0) neither, (0, 1)
    measured only, (0, 2) expected only, (0, 3) agree, (0, 4) nearer, (0, 5) farther.  The measured values are no multiples of 1/16: their
    bits must come through as they are; the fill of (0, 2) is 133 / 16."""
    d_prev, d_cur = blank(), blank()
    d_prev[0, 2] = 8.3125                                   # 133 sixteenths
    d_prev[0, 3], d_prev[0, 4], d_prev[0, 5] = 8.0, 8.0, 8.0
    d_cur[0, 1] = np.float32(5.03)
    d_cur[0, 3], d_cur[0, 4], d_cur[0, 5] = np.float32(8.03), np.float32(11.07), np.float32(3.01)
    d_cur[0, 0] = np.nan
    return d_prev, d_cur, (0, 1, 2, 3, 4, 5)


RANDOM_CAMERA = dict(SMALL, cx=18.2, cy=9.4, width=37, height=19)


def random_case(seed, shape=(19, 37), B=1, cam=None):
    """Random maps of disparities of 1 to 30 px, some invalid, under a small rotation and a translation mostly forward -> (d_prev, d_cur
    [B,H,W], poses [B,12], camera)."""
    from flow_cases import rotation
    rng = np.random.default_rng(300 + seed)
    h, w = shape
    cam = dict(RANDOM_CAMERA if cam is None else cam)
    if (h, w) != (cam["height"], cam["width"]):
        cam.update(cx=0.5 * w - 0.3, cy=0.5 * h + 0.2, width=w, height=h)
    d_prev = np.stack([noise(1000 * seed + b, 1.0, 30.0, 0.15, shape) for b in range(B)])
    d_cur = np.stack([noise(1000 * seed + 500 + b, 1.0, 30.0, 0.2, shape) for b in range(B)])
    poses = np.stack([pose_of(rotation(*rng.uniform(-0.02, 0.02, 3)), (rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03), rng.uniform(-0.5, 0.1))) for _ in range(B)])
    return d_prev, d_cur, poses, cam
