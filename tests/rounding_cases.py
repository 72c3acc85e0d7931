"""Inputs on which ONE rounding decides an integer: the few lines of double arithmetic in front of a floor() or an integer cast in the
stages that claim bit-exactness against their numpy definition, written once more as scalar models in plain Python floats - IEEE doubles,
every operation rounded on its own: the definition - and once per named mistake:

  fused:<site>    an a * b + c that a contracting compiler may fuse, evaluated exactly with fractions and rounded once; every site on its
                  own, and fused:all
  reciprocal:<site>  x * (1.0 / y) for x / y, per division
  reassociated    p0 x + (p1 y + p2 z) for (p0 x + p1 y) + p2 z
  half:rint, half:trunc  rint (ties to even) and (int)(v + 0.5) for floor(v + 0.5)

sites() draws inputs, solves one free variable so that the value in front of the floor sits beside an integer, walks it ulp by ulp and
keeps the inputs on which a mistake's integers differ from the definition's.  Random inputs show none of these mistakes: the flip is one
in 10^13 draws.  Seeds are fixed; tests/test_rounding_edges.py holds the corpora against the package's numpy definitions and runs them
through the device, translation unit by translation unit."""
import functools
import math
import random
import struct
from fractions import Fraction

import numpy as np


def fma(a, b, c):
    """a * b + c rounded once."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def ulps(v, k):
    """v moved by k units in the last place: k steps of nextafter, through the ordered integers of the doubles."""
    i = struct.unpack("<q", struct.pack("<d", v))[0]
    i = (i if i >= 0 else -(i & 0x7FFFFFFFFFFFFFFF)) + k
    return struct.unpack("<d", struct.pack("<q", i if i >= 0 else (-i) | -0x8000000000000000))[0]


class Ops:
    """The arithmetic of a model: the definition, or the definition with one named mistake.  A model names every fusable a * b + c and
    every division by a site; `fuse` and `recip` hold the sites (or "all") at which this arithmetic departs."""

    def __init__(self, fuse=(), recip=(), reassoc=False, half="floor"):
        self.fuse, self.recip, self.reassoc, self.half_rule = frozenset(fuse), frozenset(recip), reassoc, half

    def _fused(self, site):
        return site in self.fuse or "all" in self.fuse

    def mad(self, site, a, b, c):
        """a * b + c; c is a value that was rounded before."""
        return fma(a, b, c) if self._fused(site) else a * b + c

    def pp(self, site_a, site_b, a, x, b, y):
        """a * x + b * y: either product may fuse with the sum, not both."""
        if self._fused(site_a):
            return fma(a, x, b * y)
        if self._fused(site_b):
            return fma(b, y, a * x)
        return a * x + b * y

    def pm(self, site_a, site_b, a, x, b, y):
        """a * x - b * y."""
        if self._fused(site_a):
            return fma(a, x, -(b * y))
        if self._fused(site_b):
            return fma(-b, y, a * x)
        return a * x - b * y

    def row(self, p0, x, p1, y, p2, z, t):
        """((p0 x + p1 y) + p2 z) + t, the order of every pose and matrix row in the package.  Sites ax, by, cz."""
        if self.reassoc:
            return (p0 * x + (p1 * y + p2 * z)) + t
        return self.mad("cz", p2, z, self.pp("ax", "by", p0, x, p1, y)) + t

    def div(self, site, x, y):
        return x * (1.0 / y) if site in self.recip else x / y

    def half(self, v):
        """floor(v + 0.5) as an int."""
        if self.half_rule == "rint":
            return int(round(v))  # Python's round of a float: ties to even
        if self.half_rule == "trunc":
            return int(v + 0.5)
        return math.floor(v + 0.5)


DEFINITION = Ops()
ROW_FUSED = ("fused:ax", "fused:by", "fused:cz", "fused:all")


def mistake(name):
    kind, _, site = name.partition(":")
    if kind == "fused":
        return Ops(fuse=(site,))
    if kind == "reciprocal":
        return Ops(recip=(site,))
    if kind == "reassociated":
        return Ops(reassoc=True)
    if kind == "half":
        return Ops(half=site)
    raise KeyError(name)


def rotation(rng):
    """Nine doubles of a rotation, row-major, from a random unit quaternion: three non-zero products in every row."""
    while True:
        q = [rng.gauss(0.0, 1.0) for _ in range(4)]
        n = math.sqrt(sum(v * v for v in q))
        w, x, y, z = (v / n for v in q)
        R = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
             2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
        if min(abs(v) for v in R) > 0.05:
            return R


def sites(model, mistakes, sampler, free, walk=6, seed=0, draws=400, limit=4096):
    """The generic builder.  `sampler(rng, i)` draws an input (a dict) for site i, or None; `model.front(inp)` is the double in front of the
    floor that the site is aimed at and `model.result(inp, ops)` the stage's integers of the input (a tuple; None for an input outside the
    stage's contract or the corpus' bounds).  inp[free] - for free = None, inp[inp["free"]] - is solved (secant steps) so that front lands on inp["target"] - a whole
    number, given by the sampler - and then walked over +-walk ulps.  Kept: every input on which at least one mistake's result differs from
    the definition's, as (inp, tags), tags the names of the mistakes it discriminates.  At most `limit`: the sites drawn after it is reached
    add nothing, and the tests hold every corpus below it.

    The solve has two stages because either alone falls short: the secant steps get within some hundred ulps in a few evaluations but
    stall where the front's own rounding makes it a staircase, and the descent by 256, 64, 16, 4 and 1 ulps that ends it would take
    thousands of steps from the sampler's start.  Without the descent a quarter of the sites end some 10^-13 from their target, outside
    the walk."""
    rng = random.Random(seed)
    ops = [(name, mistake(name)) for name in mistakes]
    kept = []
    for i in range(draws):
        inp = sampler(rng, i)
        if inp is None:
            continue
        free_variable = inp["free"] if free is None else free
        at = lambda x: model.front(dict(inp, **{free_variable: x})) - inp["target"]  # noqa: E731
        a = inp[free_variable]
        fa = at(a)
        b, best = a + (1e-3 if a == 0.0 else abs(a) * 1e-3), (abs(fa), a)
        for _ in range(40):
            fb = at(b)
            if not math.isfinite(fb):
                break
            best = min(best, (abs(fb), b))
            if fb == 0.0 or fb == fa or a == b:
                break
            a, b, fa = b, b - fb * (b - a) / (fb - fa), fb
        for step in (256, 64, 16, 4, 1):  # and ulp by ulp, as long as it comes nearer
            moved = True
            while moved:
                moved = False
                for k in (-step, step):
                    c = ulps(best[1], k)
                    if abs(at(c)) < best[0]:
                        best, moved = (abs(at(c)), c), True
        b = best[1]
        if not math.isfinite(b) or best[0] > 1e-9 * max(1.0, abs(inp["target"])):
            continue
        seen = set()  # where the free variable is finer than the front, several steps give one value: one of them is kept
        for k in range(-walk, walk + 1):
            at = dict(inp, **{free_variable: ulps(b, k)})
            want = model.result(at, DEFINITION)
            if want is None:
                continue
            got = [(name, model.result(at, o)) for name, o in ops]
            if any(g is None for _, g in got):
                continue
            tags = tuple(name for name, g in got if g != want)
            if tags and len(kept) < limit and (model.front(at), tags) not in seen:
                seen.add((model.front(at), tags))
                kept.append((at, tags))
    return kept


def counts_of(corpus, mistakes):
    """{mistake: the number of inputs of the corpus that discriminate it}."""
    return {name: sum(name in tags for _, tags in corpus) for name in mistakes}


# ---------------------------------------------------------------------------------------------------------------- the voxel map's cell
# vmap_cell and vmap_offset of csrc/voxel_map_table.h: P = ((p0 x + p1 y) + p2 z) + t, kept iff lo < P < hi, t = (P - lo) / size,
# c = min(int(t), cells - 1), u = min(int((t - c) * 65536), 65535).  (t - c) * 65536 is exact and nothing is added to it: no site.

FRAMES = 64  # the poses of a corpus: a stage that takes one pose per frame gets 64 frames
VOXEL_BOX = dict(lo=(-2.1, -1.9, -0.9), hi=(1.9, 2.1, 1.5), size=0.2, capacity=16384)  # about 20 x 20 x 12 cells; 1.0 / 0.2 is off by a quarter ulp
VOXEL_MISTAKES = ROW_FUSED + ("reciprocal:cell", "reassociated")


def _cells(box):
    return [max(1, int(math.ceil((box["hi"][k] - box["lo"][k]) / box["size"]))) for k in range(3)]


class VoxelCell:
    def __init__(self, box=VOXEL_BOX):
        self.lo, self.hi, self.size, self.cells = box["lo"], box["hi"], box["size"], _cells(box)

    def world(self, inp, ops, k):
        p = inp["pose"]
        return ops.row(p[3 * k], inp["x"], p[3 * k + 1], inp["y"], p[3 * k + 2], inp["z"], p[9 + k])

    def front(self, inp):
        k = inp["axis"]
        return (self.world(inp, DEFINITION, k) - self.lo[k]) / self.size

    def result(self, inp, ops):
        """(cx, cy, cz, ux, uy, uz); None for a row that the definition or the mistake drops: the corpus stays inside the box."""
        c, u = [], []
        for k in range(3):
            P = self.world(inp, ops, k)
            if not self.lo[k] + 0.5 * self.size < P < self.hi[k] - 0.5 * self.size:
                return None
            t = ops.div("cell", P - self.lo[k], self.size)
            c.append(min(int(t), self.cells[k] - 1))
            u.append(min(int((t - float(c[k])) * 65536.0), 65535))
        return tuple(c + u)


@functools.lru_cache(None)
def voxel_poses(seed=11):
    rng = random.Random(seed)
    return tuple(tuple(rotation(rng) + [rng.uniform(-0.5, 0.5) for _ in range(3)]) for _ in range(FRAMES))


def _voxel_sampler(model):
    poses = voxel_poses()

    def draw(rng, i):
        pose = poses[i % FRAMES]
        k = rng.randrange(3)
        w = [rng.uniform(model.lo[a] + 2 * model.size, model.hi[a] - 2 * model.size) for a in range(3)]  # a world point well inside the box
        d = [w[a] - pose[9 + a] for a in range(3)]
        x, y, z = (pose[a] * d[0] + pose[3 + a] * d[1] + pose[6 + a] * d[2] for a in range(3))  # R^T (w - t)
        return dict(pose=pose, frame=i % FRAMES, axis=k, x=x, y=y, z=z, target=float(round((w[k] - model.lo[k]) / model.size)))
    return draw


@functools.lru_cache(None)
def voxel_corpus():
    model = VoxelCell()
    return sites(model, VOXEL_MISTAKES, _voxel_sampler(model), "z", seed=101, draws=700)


def frames_of(corpus, columns=("x", "y", "z")):
    """The rows of a corpus by frame: (xyz float64 [FRAMES,cap,3], counts int32 [FRAMES], poses float64 [FRAMES,12], where: the (frame, row)
    of every input)."""
    rows = [[] for _ in range(FRAMES)]
    where = []
    for inp, _ in corpus:
        where.append((inp["frame"], len(rows[inp["frame"]])))
        rows[inp["frame"]].append([inp[c] for c in columns])
    cap = max(len(r) for r in rows)
    xyz = np.zeros((FRAMES, cap, 3))
    for b, r in enumerate(rows):
        if r:
            xyz[b, :len(r)] = r
    return xyz, np.array([len(r) for r in rows], np.int32), np.array(voxel_poses()), where


def voxel_fill(box=VOXEL_BOX, seed=3):
    """A call (xyz, color, n, counts, poses) that puts one row into every cell of the box under the identity: a dense map, in which every
    cell a row or a sight line reaches holds a voxel."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = _cells(box)
    c = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    xyz = np.array(box["lo"]) + (c + rng.uniform(0.2, 0.8, c.shape)) * box["size"]
    return (xyz[None], None, None, np.array([len(xyz)], np.int32), np.array([[1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]]))


def thinned(corpus, mistakes, per=40):
    """The first inputs of a corpus that give every mistake `per` discriminating ones: for the stages that take one call per input."""
    have, out = dict.fromkeys(mistakes, 0), []
    for inp, tags in corpus:
        if any(have[t] < per for t in tags):
            out.append((inp, tags))
            for t in tags:
                have[t] += 1
    return out


# ---------------------------------------------------------------------------------------------------------------- the reprojected pixel
# sv_reproject_point of csrc/reproject.h under a rectified Q - rows (1, 0, 0, -cx), (0, 1, 0, -cy), (0, 0, 0, f), (0, 0, q32, 0): one
# non-zero product per row, which no fusing changes - and a full rotation XR: (X, Y, Z) = (i - cx, j - cy, f) / (q32 d), then
# ((XR_k0 X + XR_k1 Y) + XR_k2 Z) + XT_k.  Behind it the top view's and the occupancy grid's cell, trunc(x1 s) - trunc(X s) - a product
# and nothing added -, or the voxel cloud's, (P - lo) / size.  Q, XR and XT are words of the call: every input is a call of its own, one
# small image with one valid pixel.

REPROJECT_CAM = dict(f=5.25, cx=3.7, cy=2.6, q32=1.0 / 54.0)  # a toy camera: X, Y and Z of a pixel are of one magnitude, so every product of a row counts
REPROJECT_SHAPE = (6, 8)  # H, W
REPROJECT_MISTAKES = ROW_FUSED + ("reciprocal:w", "reassociated")
GRID = dict(x_range=(-16, 16), y_range=(-16, 16), z_range=(-40.0, 40.0), scale=3)
CLOUD_BOX = dict(lo=(-16.1, -15.9, -16.3), hi=(15.9, 16.1, 15.7), size=0.2)
CLOUD_MISTAKES = REPROJECT_MISTAKES + ("reciprocal:cell",)


def reproject_q(cam=REPROJECT_CAM):
    return np.array([[1.0, 0, 0, -cam["cx"]], [0, 1.0, 0, -cam["cy"]], [0, 0, 0, cam["f"]], [0, 0, cam["q32"], 0]])


class Reprojected:
    def __init__(self, kind, cam=REPROJECT_CAM):
        self.kind, self.cam = kind, cam
        self.box = VoxelCell(dict(CLOUD_BOX, capacity=1))

    def point(self, inp, ops):
        i, j, d = inp["i"], inp["j"], inp["d"]
        w = self.cam["q32"] * d
        X, Y, Z = (ops.div("w", v, w) for v in (float(i) - self.cam["cx"], float(j) - self.cam["cy"], self.cam["f"]))
        R = inp["XR"]
        return [ops.row(R[3 * k], X, R[3 * k + 1], Y, R[3 * k + 2], Z, inp["t%d" % k]) for k in range(3)]

    def front(self, inp):
        k = inp["axis"]
        P = self.point(inp, DEFINITION)[k]
        return P * GRID["scale"] if self.kind == "grid" else (P - self.box.lo[k]) / self.box.size

    def result(self, inp, ops):
        """(row, col) of the grid, or the voxel's cell and offsets.  None where the point leaves the ranges."""
        P = self.point(inp, ops)
        if self.kind == "grid":
            if not all(-15.5 < v < 15.5 for v in P):
                return None
            s = float(GRID["scale"])
            return (int(GRID["x_range"][1] * s) - int(P[0] * s), int(GRID["y_range"][1] * s) - int(P[1] * s))
        c = []
        for k in range(3):
            if not self.box.lo[k] + 0.5 < P[k] < self.box.hi[k] - 0.5:
                return None
            t = ops.div("cell", P[k] - self.box.lo[k], self.box.size)
            c.append(min(int(t), self.box.cells[k] - 1))
            c.append(min(int((t - float(c[-1])) * 65536.0), 65535))
        return tuple(c)


def _reproject_sampler(kind):
    def draw(rng, n):
        H, W = REPROJECT_SHAPE
        i, j, XR, k = rng.randrange(W), rng.randrange(H), rotation(rng), rng.randrange(2 if kind == "grid" else 3)
        inp = dict(i=i, j=j, d=float(np.float32(rng.uniform(24.0, 40.0))), XR=XR, axis=k, free="t%d" % k, t0=0.0, t1=0.0, t2=0.0)
        P = Reprojected(kind).point(inp, DEFINITION)
        w = [rng.uniform(-3.0, 3.0) for _ in range(3)]  # where the aimed pixel shall lie
        inp.update({"t%d" % a: w[a] - P[a] for a in range(3)})
        if kind == "grid":
            inp["target"] = float(round(w[k] * GRID["scale"]))
        else:
            inp["target"] = float(round((w[k] - CLOUD_BOX["lo"][k]) / CLOUD_BOX["size"]))
        return inp
    return draw


@functools.lru_cache(None)
def reproject_corpus(kind):
    mistakes = REPROJECT_MISTAKES if kind == "grid" else CLOUD_MISTAKES
    return thinned(sites(Reprojected(kind), mistakes, _reproject_sampler(kind), None, seed=202 if kind == "grid" else 203, draws=400), mistakes)


def reproject_call(inp):
    """(d float32 [1,H,W], Q, XR [3,3], XT [3]) of an input."""
    d = np.full((1,) + REPROJECT_SHAPE, -1.0, np.float32)
    d[0, inp["j"], inp["i"]] = inp["d"]
    return d, reproject_q(), np.array(inp["XR"]).reshape(3, 3), np.array([inp["t0"], inp["t1"], inp["t2"]])


# ---------------------------------------------------------------------------------------------------------------- the flat map's cell
# map_world, map_grid and map_cell of csrc/occupancy_map_cells.h: Xw = (c X - s Y) + tx, Yw = (s X + c Y) + ty, gx = floor(Xw ms), cell
# (top - 1 - gx, left - 1 - gy): two products per row, sites ax and by (a compiler fuses one of them; fused:all is fused:ax).  No division.
# The fuse goes the other way (occupancy_map_kernels.hip): dx = Xw - tx, dy = Yw - ty, Xf = c dx + s dy, Yf = c dy - s dx, frame cell
# (trunc(fx1 fs) - trunc(Xf fs), trunc(fy1 fs) - trunc(Yf fs)).

FLAT_MISTAKES = ("fused:ax", "fused:by", "fused:all")
FLAT_FRAME = dict(x_range=(0, 4), y_range=(-2, 2), scale=3)  # 13 x 13 cells; the points of its cells are sixths
FLAT_MAP = dict(x_range=(-6, 10), y_range=(-8, 8), scale=5)  # 80 x 80 cells
FUSE_MAP = dict(x_range=(-2, 4), y_range=(-3, 3), scale=4, l_occ=3, l_free=2, l_min=-32767, l_max=32767)  # 24 x 24 cells, a clamp no sum reaches
MATCH_FRAMES = 16
DISC = (1.3, -0.7)  # the one disc of the path check's footprint


def frame_point(k, fs):
    """The point a frame cell with k = trunc(f1 fs) - index stands for: occupancy_frame_points' rule."""
    return float(2 * k + (k > 0) - (k < 0)) * (1.0 / (2.0 * fs))


class FlatCell:
    """A vehicle point under a pose into the map: inp has X, Y, tx, ty, c, s."""

    def __init__(self, grid=FLAT_MAP):
        s = grid["scale"]
        self.ms, self.top, self.left = float(s), grid["x_range"][1] * s, grid["y_range"][1] * s
        self.rows, self.cols = (grid["x_range"][1] - grid["x_range"][0]) * s, (grid["y_range"][1] - grid["y_range"][0]) * s

    def world(self, inp, ops):
        return ops.pm("ax", "by", inp["c"], inp["X"], inp["s"], inp["Y"]) + inp["tx"], ops.pp("ax", "by", inp["s"], inp["X"], inp["c"], inp["Y"]) + inp["ty"]

    def front(self, inp):
        return self.world(inp, DEFINITION)[inp["axis"]] * self.ms

    def result(self, inp, ops):
        gx, gy = (math.floor(v * self.ms) for v in self.world(inp, ops))
        r, c = self.top - 1 - gx, self.left - 1 - gy
        return (r, c) if 2 <= r < self.rows - 2 and 2 <= c < self.cols - 2 else None


class FuseBack:
    """A map cell's centre under a frame's pose back into the frame grid: inp has Xw, Yw, tx, ty, c, s."""

    def __init__(self, frame=FLAT_FRAME):
        self.fs, self.fx, self.fy = float(frame["scale"]), frame["x_range"], frame["y_range"]

    def frame(self, inp, ops):
        dx, dy = inp["Xw"] - inp["tx"], inp["Yw"] - inp["ty"]
        return ops.pp("ax", "by", inp["c"], dx, inp["s"], dy), ops.pm("ax", "by", inp["c"], dy, inp["s"], dx)

    def front(self, inp):
        return self.frame(inp, DEFINITION)[inp["axis"]] * self.fs

    def result(self, inp, ops):
        Xf, Yf = self.frame(inp, ops)
        if not (self.fx[0] + 0.4 < Xf < self.fx[1] - 0.4 and self.fy[0] + 0.4 < Yf < self.fy[1] - 0.4):
            return None
        return int(self.fx[1] * self.fs) - int(Xf * self.fs), int(self.fy[1] * self.fs) - int(Yf * self.fs)


def _yaw(rng):
    while True:
        yaw = rng.uniform(-math.pi, math.pi)
        c, s = float(np.cos(yaw)), float(np.sin(yaw))
        if min(abs(c), abs(s)) > 0.1:
            return c, s


@functools.lru_cache(None)
def match_cells(seed=31):
    """(fr, fc) of the one occupied cell of each of the match's frames, off the double-width cells at 0."""
    rng = random.Random(seed)
    n = FLAT_FRAME["scale"] * 4 + 1
    return tuple((rng.randrange(0, n - 2), rng.choice([c for c in range(n) if c != n // 2])) for _ in range(MATCH_FRAMES))


def _flat_sampler(point_of):
    def draw(rng, i):
        c, s = _yaw(rng)
        X, Y = point_of(i)
        k = rng.randrange(2)
        inp = dict(site=i, X=X, Y=Y, c=c, s=s, tx=rng.uniform(-2.0, 2.0), ty=rng.uniform(-2.0, 2.0), axis=k, free=("tx", "ty")[k])
        inp["target"] = float(round(FlatCell().front(inp)))
        return inp
    return draw


def _match_point(i):
    fr, fc = match_cells()[i % MATCH_FRAMES]
    fs = FLAT_FRAME["scale"]
    return frame_point(FLAT_FRAME["x_range"][1] * fs - fr, fs), frame_point(FLAT_FRAME["y_range"][1] * fs - fc, fs)


@functools.lru_cache(None)
def match_corpus():
    return sites(FlatCell(), FLAT_MISTAKES, _flat_sampler(_match_point), None, seed=301, draws=500)


@functools.lru_cache(None)
def clearance_corpus():
    return sites(FlatCell(), FLAT_MISTAKES, _flat_sampler(lambda i: DISC), None, seed=302, draws=500)


def pose4(inp):
    return [inp["tx"], inp["ty"], inp["c"], inp["s"]]


def flat_match_call(corpus):
    """(state uint8 [16,13,13], poses float64 [16,P,4], where: (frame, candidate) of every input); a frame's row of candidates is filled up
    with its first."""
    n = FLAT_FRAME["scale"] * 4 + 1
    state = np.zeros((MATCH_FRAMES, n, n), np.uint8)
    for b, (fr, fc) in enumerate(match_cells()):
        state[b, fr, fc] = 2
    rows = [[] for _ in range(MATCH_FRAMES)]
    where = []
    for inp, _ in corpus:
        b = inp["site"] % MATCH_FRAMES
        where.append((b, len(rows[b])))
        rows[b].append(pose4(inp))
    P = max(len(r) for r in rows)
    assert min(len(r) for r in rows) > 0
    return state, np.array([r + [r[0]] * (P - len(r)) for r in rows]), where


def unique_cells(rows, cols, dtype):
    """A field in which every cell holds another number: what a lookup returns names its cell."""
    return (np.arange(rows * cols).reshape(rows, cols) - (rows * cols // 2 if np.dtype(dtype).kind == "i" else 0)).astype(dtype)


def _fuse_sampler(rng, i):
    s = FUSE_MAP["scale"]
    rows, cols = (FUSE_MAP["x_range"][1] - FUSE_MAP["x_range"][0]) * s, (FUSE_MAP["y_range"][1] - FUSE_MAP["y_range"][0]) * s
    r, cc, half = rng.randrange(rows), rng.randrange(cols), 1.0 / (2.0 * s)
    c, sn = _yaw(rng)
    k = rng.randrange(2)
    inp = dict(r=r, col=cc, Xw=float(2 * (FUSE_MAP["x_range"][1] * s - r) - 1) * half, Yw=float(2 * (FUSE_MAP["y_range"][1] * s - cc) - 1) * half, c=c, s=sn,
               tx=rng.uniform(-1.0, 1.0), ty=rng.uniform(-1.0, 1.0), axis=k, free=("tx", "ty")[k])
    model = FuseBack()
    if model.result(inp, DEFINITION) is None:
        return None
    inp["target"] = float(round(model.front(inp)))
    return inp if inp["target"] != 0.0 else None


@functools.lru_cache(None)
def fuse_corpus():
    return thinned(sites(FuseBack(), FLAT_MISTAKES, _fuse_sampler, None, seed=303, draws=1500), FLAT_MISTAKES, per=64)


def fuse_state(B):
    """uint8 [B,13,13]: free and occupied cells in a chequerboard, so that a point one cell off reads the other state."""
    n = FLAT_FRAME["scale"] * 4 + 1
    i = np.arange(n)
    return np.broadcast_to((1 + (i[:, None] + i[None, :]) % 2).astype(np.uint8), (B, n, n)).copy()


# ---------------------------------------------------------------------------------------------------------------- the moved pixel
# flow_point of csrc/flow_point.h - X0 = (((u - cx) b16) / dq, ((v - cy) b16) / dq, fb16 / dq), then the pose's three rows - and behind it
#   warp, match   tu = floor(((f x) / z + cx) + 0.5), tv alike, pd = floor(16 (fb / z) + 0.5)   (warp_kernels.hip, k_flow_match)
#   sums          xz = x / z, pu = floor(16 (f xz + cx) + 0.5), pv alike, pd = floor(16 (fb / z) + 0.5)   (k_flow_score)
# A multiplication by 16 is exact, so 16 q + 0.5 fused is the same number: fused:sixteen is listed and must discriminate nothing.  The
# pixel and its disparity are integers and the pose is one per frame: every input is a frame of its own, with one pixel, match or point.

MOVED_CAM = dict(f=41.3, cx=15.7, cy=11.4, q32=1.0 / 0.53, q33=0.0, width=32, height=24, size=1.0, half_px=0.0)  # voxel_render_camera's words; nothing dyadic
EDGE_CAM = dict(MOVED_CAM, cx=0.3)  # u + cx of a pixel near the left rim is a sum of two small numbers: it reaches 0.5 - 2^-54, which + 0.5 rounds up to 1
MOVED_SHAPE = (24, 32)  # H, W
HALF = ("half:rint", "half:trunc")
WARP_MISTAKES = ROW_FUSED + ("reassociated", "reciprocal:point", "reciprocal:proj", "reciprocal:depth") + HALF
SUMS_MISTAKES = ROW_FUSED + ("reassociated", "reciprocal:point", "reciprocal:proj", "reciprocal:depth", "fused:proj") + HALF
MOVED_NONE = ("fused:sixteen",)
Z_MIN = 0.5  # the corpus keeps its points well in front of FLOW_Z_MIN


def moved_camera(cam=MOVED_CAM):
    """sv.flow_camera's products."""
    b = 1.0 / cam["q32"]
    b16 = 16.0 * b
    return dict(f=cam["f"], cx=cam["cx"], cy=cam["cy"], b16=b16, fb=cam["f"] * b, fb16=cam["f"] * b16)


class Moved:
    def __init__(self, kind, cam=MOVED_CAM):
        self.kind, self.cam = kind, moved_camera(cam)

    def point(self, inp, ops):
        c, d = self.cam, float(inp["dq"])
        x0, y0, z0 = ops.div("point", (float(inp["u"]) - c["cx"]) * c["b16"], d), ops.div("point", (float(inp["v"]) - c["cy"]) * c["b16"], d), ops.div("point", c["fb16"], d)
        R = inp["R"]
        return [ops.row(R[3 * k], x0, R[3 * k + 1], y0, R[3 * k + 2], z0, inp["t%d" % k]) for k in range(3)]

    def values(self, inp, ops):
        """The three doubles in front of the + 0.5: u, v and disparity."""
        c = self.cam
        x, y, z = self.point(inp, ops)
        if not z > Z_MIN:
            return None
        bz = ops.mad("sixteen", 16.0, ops.div("depth", c["fb"], z), 0.0)  # the + 0.5 is half()'s: fused or not, 16 q is exact
        if self.kind == "sums":
            return [16.0 * ops.mad("proj", c["f"], ops.div("proj", v, z), o) for v, o in ((x, c["cx"]), (y, c["cy"]))] + [bz]
        return [ops.div("proj", c["f"] * v, z) + o for v, o in ((x, c["cx"]), (y, c["cy"]))] + [bz]

    def front(self, inp):
        v = self.values(inp, DEFINITION)
        return math.nan if v is None else v[inp["axis"]] + 0.5

    def result(self, inp, ops):
        v = self.values(inp, ops)
        if v is None:
            return None
        pu, pv, pd = (ops.half(a) for a in v)
        if not 1 <= pd <= 2 ** 20:
            return None
        if self.kind == "sums":
            return pu, pv, pd
        if self.kind == "match":
            return match_at(pu, pv)
        H, W = MOVED_SHAPE
        e = min(1, (pd + inp["dq"] - 1) // inp["dq"] - 1)
        return (pd,) + tuple((pv + dy, pu + dx) for dy in range(e + 1) for dx in range(e + 1) if 0 <= pv + dy < H and 0 <= pu + dx < W)


def moved_mistakes(kind):
    return SUMS_MISTAKES if kind == "sums" else tuple(m for m in WARP_MISTAKES if kind == "warp" or m != "reciprocal:depth")


def moved_none(kind):
    """What provably changes nothing: 16 q + 0.5 fused, and for the matcher, which does not use the disparity, fb / z."""
    return MOVED_NONE + (("reciprocal:depth",) if kind == "match" else ())


def small_rotation(rng, most=0.3):
    a, b, c = (rng.uniform(-most, most) for _ in range(3))
    ca, sa, cb, sb, cc, sc = math.cos(a), math.sin(a), math.cos(b), math.sin(b), math.cos(c), math.sin(c)
    return [cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa, sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa, -sb, cb * sa, cb * ca]


def _moved_sampler(kind, cam=MOVED_CAM):
    H, W = MOVED_SHAPE

    def draw(rng, i):
        if kind == "match":
            u, v = MATCH_POINT
        else:
            u, v = rng.randrange(W), rng.randrange(H)
        k = rng.randrange(2 if kind == "match" else 3)
        inp = dict(u=u, v=v, dq=int(math.floor(16.0 * float(np.float32(rng.uniform(2.0, 12.0))) + 0.5)), R=small_rotation(rng, rng.choice((0.3, 0.03))), axis=k, free="t%d" % k,
                   t0=rng.uniform(-0.3, 0.3), t1=rng.uniform(-0.3, 0.3), t2=rng.uniform(-0.3, 0.3))
        if cam is EDGE_CAM:
            inp.update(axis=0, free="t0")
        at = Moved(kind, cam).front(inp)
        if not math.isfinite(at):
            return None
        inp["target"] = 1.0 if cam is EDGE_CAM else float(round(at))
        if cam is not EDGE_CAM and k < 2 and i % 4 == 0:  # the left and the upper rim and beyond: floor and truncation part below zero
            inp["target"] = float(1 - rng.randrange(0, 200) if kind == "sums" else 1 - rng.randrange(0, 4))  # 1: v = 0.5 - 2^-54, which + 0.5 rounds up
        return inp
    return draw


@functools.lru_cache(None)
def moved_corpus(kind):
    mistakes = moved_mistakes(kind) + moved_none(kind)
    return sites(Moved(kind), mistakes, _moved_sampler(kind), None, seed=dict(warp=401, sums=402, match=403)[kind], draws=dict(warp=1000, sums=600, match=1500)[kind])


ROUNDS_UP = 0.49999999999999994  # 0.5 - 2^-54


@functools.lru_cache(None)
def edge_corpus():
    """The warp under EDGE_CAM, aimed at column 0 | 1: the inputs whose u is exactly ROUNDS_UP, which rint sends to column 0."""
    model = Moved("warp", EDGE_CAM)
    found = sites(model, HALF, _moved_sampler("warp", EDGE_CAM), None, walk=24, seed=411, draws=500)
    return [(inp, tags) for inp, tags in found if model.values(inp, DEFINITION)[0] == ROUNDS_UP]


def moved_pose(inp):
    return list(inp["R"]) + [inp["t0"], inp["t1"], inp["t2"]]


def warp_call(corpus):
    """(d_prev float32 [B,24,32] with one valid pixel per frame, poses [B,12])."""
    d = np.full((len(corpus),) + MOVED_SHAPE, -1.0, np.float32)
    for b, (inp, _) in enumerate(corpus):
        d[b, inp["v"], inp["u"]] = inp["dq"] / 16.0
    return d, np.array([moved_pose(inp) for inp, _ in corpus])


def sums_call(corpus):
    """(matches int32 [B,1,6], counts int32 [B], poses [B,12]): one match per frame, its target the nearest whole pixel and disparity."""
    model = Moved("sums")
    rows = []
    for inp, _ in corpus:
        pu, pv, pd = model.result(inp, DEFINITION)
        rows.append([[inp["u"], inp["v"], inp["dq"], (pu + 8) // 16, (pv + 8) // 16, pd + 1]])
    return np.array(rows, np.int32), np.ones(len(corpus), np.int32), np.array([moved_pose(inp) for inp, _ in corpus])


# flow_match under a guess shows the centre only through which window is searched.  prev and cur are two fixed random textures, the same in
# every frame, with one lattice point that has a disparity; the model runs the matcher's rule on the window around the centre it gets, so
# an input is kept only where the mistaken centre changes the match itself: (u1, v1), best, second, or whether there is one.

MATCH_POINT = (24, 16)
MATCH_WORDS = dict(step=8, r=1, wx=4, wy=4, ratio=256, capacity=1)


@functools.lru_cache(None)
def match_texture(seed=7):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, MOVED_SHAPE).astype(np.uint8), rng.integers(0, 256, MOVED_SHAPE).astype(np.uint8)


@functools.lru_cache(None)
def match_at(ccx, ccy):
    """flow_match's rule for the one point MATCH_POINT with the centre (ccx, ccy): (u1, v1, best, second), or () for no match."""
    prev, cur = (t.astype(np.int64) for t in match_texture())
    (H, W), (u0, v0) = MOVED_SHAPE, MATCH_POINT
    r, wx, wy = MATCH_WORDS["r"], MATCH_WORDS["wx"], MATCH_WORDS["wy"]
    patch = prev[v0 - r:v0 + r + 1, u0 - r:u0 + r + 1]
    cost = {}
    for dy in range(-wy, wy + 1):
        for dx in range(-wx, wx + 1):
            x, y = ccx + dx, ccy + dy
            if r <= x < W - r and r <= y < H - r:
                cost[(dy, dx)] = int(np.abs(cur[y - r:y + r + 1, x - r:x + r + 1] - patch).sum())
    if not cost:
        return ()
    best = min(cost, key=lambda k: (cost[k], k))
    rest = [c for k, c in cost.items() if max(abs(k[0] - best[0]), abs(k[1] - best[1])) > 1]
    if not rest or not 256 * cost[best] < MATCH_WORDS["ratio"] * min(rest) or abs(best[1]) == wx or abs(best[0]) == wy:
        return ()
    return ccx + best[1], ccy + best[0], cost[best], min(rest)


def match_call(corpus):
    """(prev, cur uint8 [B,24,32], d_prev float32 [B,24,32], guess [B,12])."""
    B = len(corpus)
    prev, cur = (np.broadcast_to(t, (B,) + MOVED_SHAPE).copy() for t in match_texture())
    d = np.full((B,) + MOVED_SHAPE, -1.0, np.float32)
    for b, (inp, _) in enumerate(corpus):
        d[b, MATCH_POINT[1], MATCH_POINT[0]] = inp["dq"] / 16.0
    return prev, cur, d, np.array([moved_pose(inp) for inp, _ in corpus])



# ---------------------------------------------------------------------------------------------------------------- a voxel's centre
# vmap_centre of csrc/voxel_map_table.h: lo + (c + (S + 0.5 n) / (65536 n)) * size - one fusable product (site centre), one division (site
# centre); 0.5 n and S + 0.5 n are exact.  The render and the flatten read it in front of their own rules.  A voxel here is two rows of
# weights 3 and 4 in one cell, at `rel` = (c + (u + 0.5) / 65536) * size from lo: n = 7, so the quotient is not exact, and the rows' own
# cells and offsets, half a unit inside theirs, do not move when lo is walked by ulps.

CENTRE_WEIGHTS = (3, 4)
CENTRE_MISTAKES = ("fused:centre", "reciprocal:centre")
IDENTITY12 = [1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


def voxel_rows(lo, rels):
    """The two rows of a voxel: lo + rel per axis, as the call and the model both compute them."""
    return [[lo[k] + rel[k] for k in range(3)] for rel in rels]


def voxel_centre(lo, size, cells, rels, ops):
    """The centre of the voxel the two rows make, under `ops`; the rows' cells and offsets are the insert's: the definition's."""
    out = []
    for k in range(3):
        S = n = 0
        for p, w in zip(voxel_rows(lo, rels), CENTRE_WEIGHTS):
            t = (p[k] - lo[k]) / size
            c = min(int(t), cells[k] - 1)
            S, n = S + w * min(int((t - float(c)) * 65536.0), 65535), n + w
        out.append(ops.mad("centre", float(c) + ops.div("centre", float(S) + 0.5 * float(n), 65536.0 * float(n)), size, lo[k]))
    return out


def draw_rels(rng, size, cells):
    """Two rows in one cell, each half an offset unit inside its 1 / 65536."""
    c = [rng.randrange(2, cells[k] - 2) for k in range(3)]
    return tuple(tuple((c[k] + (rng.randrange(1000, 64000) + 0.5) / 65536.0) * size for k in range(3)) for _ in CENTRE_WEIGHTS)


def centre_call(lo, rels):
    """The insert's call (xyz, color, n, counts, poses) that makes the voxel."""
    return (np.array(voxel_rows(lo, rels))[None], None, np.array([CENTRE_WEIGHTS], np.int32), np.array([len(CENTRE_WEIGHTS)], np.int32), np.array([IDENTITY12]))


# ---------------------------------------------------------------------------------------------------------------- the rendered voxel
# vrender_square of csrc/voxel_render_kernels.hip behind vmap_centre: Pc = the view's three rows, tz = Pc.z / size, zq = int(tz * 256),
# u = (f Pc.x) / Pc.z + cx, px = floor(u + 0.5), r = int(half_px / tz).  A view renders the whole map, so a map holds one voxel and every
# view of it is an input, its translation the free variable; RENDER_MAPS maps, each voxel chosen so that its centre is another double
# under fused:centre and under reciprocal:centre.

RENDER_MAPS = 8
RENDER_CAM = dict(f=41.4, cx=7.7, cy=5.4, q32=1.0 / 0.53, q33=0.0, half_px=20.7, width=16, height=12)
RENDER_MISTAKES = ROW_FUSED + ("reassociated",) + CENTRE_MISTAKES + ("reciprocal:tz", "reciprocal:proj", "reciprocal:r") + HALF
R_MAX = 4


class Rendered:
    def __init__(self, box=VOXEL_BOX, cam=RENDER_CAM):
        self.lo, self.size, self.cells, self.cam = box["lo"], box["size"], _cells(box), cam

    def values(self, inp, ops):
        """(tz * 256, u, v, half_px / tz) of the view."""
        P, R, c = voxel_centre(self.lo, self.size, self.cells, inp["rels"], ops), inp["R"], self.cam
        Pc = [ops.row(R[3 * k], P[0], R[3 * k + 1], P[1], R[3 * k + 2], P[2], inp["t%d" % k]) for k in range(3)]
        tz = ops.div("tz", Pc[2], self.size)
        if not 2.0 <= tz < 1000.0:
            return None
        return [tz * 256.0, ops.div("proj", c["f"] * Pc[0], Pc[2]) + c["cx"], ops.div("proj", c["f"] * Pc[1], Pc[2]) + c["cy"], ops.div("r", c["half_px"], tz)]

    def front(self, inp):
        v = self.values(inp, DEFINITION)
        return math.nan if v is None else v[inp["axis"]] + (0.5 if inp["axis"] in (1, 2) else 0.0)

    def result(self, inp, ops):
        """(zq, x0, x1, y0, y1): the depth and the square, clipped to the image; None for a voxel that is not drawn."""
        v = self.values(inp, ops)
        if v is None:
            return None
        W, H = self.cam["width"], self.cam["height"]
        px, py, r = ops.half(v[1]), ops.half(v[2]), R_MAX if v[3] >= R_MAX else int(v[3])
        x0, x1, y0, y1 = max(px - r, 0), min(px + r, W - 1), max(py - r, 0), min(py + r, H - 1)
        return (int(v[0]), x0, x1, y0, y1) if x0 <= x1 and y0 <= y1 else None


@functools.lru_cache(None)
def render_voxels(seed=51):
    """The voxels (their rows' rel) of the RENDER_MAPS maps."""
    rng, m, out = random.Random(seed), Rendered(), []
    for _ in range(10000):
        rels = draw_rels(rng, m.size, m.cells)
        if all(voxel_centre(m.lo, m.size, m.cells, rels, mistake(x)) != voxel_centre(m.lo, m.size, m.cells, rels, DEFINITION) for x in CENTRE_MISTAKES):
            out.append(rels)
            if len(out) == RENDER_MAPS:
                return tuple(out)
    raise AssertionError("no voxels whose centre both mistakes move")


def _render_sampler(rng, i):
    model = Rendered()
    rels, R, k = render_voxels()[i % RENDER_MAPS], small_rotation(rng, rng.choice((0.3, 0.03))), rng.randrange(4)
    z = rng.uniform(1.0, 3.6)
    want = [(rng.uniform(1.0, 14.0) - RENDER_CAM["cx"]) * z / RENDER_CAM["f"], (rng.uniform(1.0, 10.0) - RENDER_CAM["cy"]) * z / RENDER_CAM["f"], z]
    P = voxel_centre(model.lo, model.size, model.cells, rels, DEFINITION)
    inp = dict(map=i % RENDER_MAPS, rels=rels, R=R, axis=k, free="t%d" % (2 if k in (0, 3) else k - 1))
    inp.update({"t%d" % a: want[a] - ((R[3 * a] * P[0] + R[3 * a + 1] * P[1]) + R[3 * a + 2] * P[2]) for a in range(3)})
    at = model.front(inp)
    if not math.isfinite(at):
        return None
    inp["target"] = float(round(at))
    if k in (1, 2) and i % 4 == 0:  # the left and the upper rim: floor and truncation part below zero
        inp["target"] = float(1 - rng.randrange(0, 4))
    return inp if inp["target"] != 0.0 or k in (1, 2) else None


@functools.lru_cache(None)
def render_corpus():
    return sites(Rendered(), RENDER_MISTAKES, _render_sampler, None, seed=501, draws=1000)


def render_calls(corpus):
    """Per map: (the insert's call, cams float64 [V,12], the indices of its inputs in the corpus)."""
    out = []
    for m, rels in enumerate(render_voxels()):
        at = [i for i, (inp, _) in enumerate(corpus) if inp["map"] == m]
        out.append((centre_call(VOXEL_BOX["lo"], rels), np.array([moved_pose(corpus[i][0]) for i in at]), at))
    return out


# ---------------------------------------------------------------------------------------------------------------- the flattened voxel
# voxel_flatten_kernels.hip: X, Y = vmap_centre on axes 0 and 1, gx = floor(X ms), flat cell (top - 1 - gx, left - 1 - gy): map_grid and
# map_cell.  The voxel's words are integers; what is a double is the voxel map's own lo, a word of the call, and the rows lie at lo + rel:
# lo on the aimed axis is the free variable, and every input is a voxel map and a call of its own.

FLATTEN_MAP = dict(x_range=(-4, 4), y_range=(-4, 4), scale=5)  # 40 x 40 cells
FLATTEN_CELLS = (16, 16, 8)
FLATTEN_SIZE = 0.2


def flatten_box(inp):
    lo = (inp["lo0"], inp["lo1"], inp["lo2"])
    return dict(lo=lo, hi=tuple(lo[k] + (FLATTEN_CELLS[k] - 0.5) * FLATTEN_SIZE for k in range(3)), size=FLATTEN_SIZE, capacity=512)


class Flattened:
    def __init__(self):
        self.flat = FlatCell(FLATTEN_MAP)

    def centre(self, inp, ops):
        return voxel_centre((inp["lo0"], inp["lo1"], inp["lo2"]), FLATTEN_SIZE, FLATTEN_CELLS, inp["rels"], ops)

    def front(self, inp):
        return self.centre(inp, DEFINITION)[inp["axis"]] * self.flat.ms

    def result(self, inp, ops):
        if _cells(flatten_box(inp)) != list(FLATTEN_CELLS):
            return None
        X, Y, _ = self.centre(inp, ops)
        r, c = self.flat.top - 1 - math.floor(X * self.flat.ms), self.flat.left - 1 - math.floor(Y * self.flat.ms)
        return (r, c) if 0 <= r < self.flat.rows and 0 <= c < self.flat.cols else None


def _flatten_sampler(rng, i):
    k = rng.randrange(2)
    inp = dict(rels=draw_rels(rng, FLATTEN_SIZE, FLATTEN_CELLS), lo0=rng.uniform(-3.9, 0.5), lo1=rng.uniform(-3.9, 0.5), lo2=rng.uniform(-1.0, 0.0), axis=k, free="lo%d" % k)
    inp["target"] = float(round(Flattened().front(inp)))
    return inp


@functools.lru_cache(None)
def flatten_corpus():
    return thinned(sites(Flattened(), CENTRE_MISTAKES, _flatten_sampler, None, seed=601, draws=1700), CENTRE_MISTAKES, per=40)
