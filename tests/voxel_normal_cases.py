"""Inputs for the normals of the voxel map and the point-to-plane sums (group (Y)).  The maps come from voxel_map_cases, voxel_align_cases
and voxel_match_cases; the independent models are stereo_vision.sv.voxel_map_normals_brute and voxel_map_align_plane_sums_brute, Python
loops over all voxels in Python ints and fractions."""
import functools

import numpy as np

import voxel_align_cases as acases
import voxel_map_cases as cases
from voxel_map_cases import BOX16

NORMAL_FIELDS = ("normal", "fit", "counts", "key")
PLANE_FIELDS = ("sums", "pair_key", "pair_d2", "pair_normal")
DTYPES = dict(normal=np.int32, fit=np.int64, counts=np.int64, key=np.int64, sums=np.int64, pair_key=np.int64, pair_d2=np.int32, pair_normal=np.int32)
AXES = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.int8)  # Q / s = C00, C11, C22
FILTERS = (dict(), dict(min_rows=2), dict(min_n=3, since=0))
STREET_BOX = dict(lo=(0.0, -4.0, -0.5), hi=(20.0, 4.0, 3.5), size=0.2, capacity=16384)  # 100 x 40 x 20 cells


def same(got, want, fields):
    """Shape, dtype and bits of every field."""
    for k in fields:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.dtype != DTYPES[k] or a.tobytes() != b.tobytes():
            return False
    return True


def at_sub(cell, sub):
    """A point whose row lands in `cell` of a map of unit cells from 0 with the offsets sub (0 .. 255 per axis, in 1/256 of a cell)."""
    return np.asarray(cell, np.float64) + (np.asarray(sub, np.float64) + 0.5) / 256.0


def one_voxel_each(points):
    """A call that inserts every point as a voxel of its own."""
    return [cases.one_frame(np.asarray(points, np.float64))]


def plate_case(axis=2):
    """A 3 x 3 plate of voxels across `axis` in BOX16, every mean at offset 128: cells 4 .. 6 on the two other axes, cell 5 on `axis`."""
    cells = []
    for u in (4, 5, 6):
        for v in (4, 5, 6):
            c = [u, v]
            c.insert(axis, 5)
            cells.append(c)
    return BOX16, one_voxel_each([at_sub(c, (128, 128, 128)) for c in cells])


def column_case():
    return BOX16, one_voxel_each([at_sub((5, 5, z), (128, 128, 128)) for z in (3, 4, 5, 6, 7)])


def flat_threshold_case():
    """Five voxels: the centre, two at e = (+-256, 0, 0) and two at e = (0, +-64, +-256).  Under AXES lam1 = 655360 (x, which ties with z and
    has the lower index), lam3 = C11 = 5 * 2 * 64^2 = 40960, lam2 = T - lam1 - lam3 = 655360: 256 lam3 = 16 lam2 exactly."""
    pts = [at_sub((5, 5, 5), (128, 128, 128)), at_sub((6, 5, 5), (128, 128, 128)), at_sub((4, 5, 5), (128, 128, 128)),
           at_sub((5, 5, 6), (128, 192, 128)), at_sub((5, 5, 4), (128, 64, 128))]
    return BOX16, one_voxel_each(pts)


def wide_threshold_case():
    """Five voxels: the centre, two at e = +-(320, 0, 64) and two at e = (0, +-280, 0).  Under AXES lam1 = 10 * 320^2 = 1024000, lam2 = 10 *
    280^2 = 784000, lam3 = 10 * 64^2 = 40960: 256 lam2 = 196 lam1 exactly."""
    pts = [at_sub((5, 5, 5), (128, 128, 128)), at_sub((6, 5, 5), (192, 128, 192)), at_sub((4, 5, 5), (64, 128, 64)),
           at_sub((5, 6, 5), (128, 152, 128)), at_sub((5, 4, 5), (128, 104, 128))]
    return BOX16, one_voxel_each(pts)


def entry_of(state, cell):
    """The index of `cell`'s voxel among the map's entries in ascending key."""
    return int(np.searchsorted(np.sort(state["key"]), acases.key_of(cell)))


def covariances(state):
    """(entries in ascending key, C float64 [M,3,3]) of the map's voxels with n >= 1, by a loop per voxel over all of them."""
    order = np.argsort(state["key"], kind="stable")
    key, n, S = state["key"][order], state["n"][order], state["S"][order]
    live = np.flatnonzero(n >= 1)
    cell = np.stack([key & 0xFFFFF, (key >> 20) & 0xFFFFF, (key >> 40) & 0xFFFFF], -1)[live]
    q = 256 * cell + ((S[live] // n[live, None]) >> 8)
    C = np.zeros((len(live), 3, 3))
    for i in range(len(live)):
        e = (q[(np.abs(cell - cell[i]) <= 1).all(1)] - q[i]).astype(np.float64)
        C[i] = len(e) * e.T @ e - np.outer(e.sum(0), e.sum(0))
    return live, C


def covering_radius(dirs, samples=20000, seed=3):
    """The largest angle, degrees, between one of `samples` random directions and the nearest line of the table: a sample of the table's
    covering radius, from below."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(samples, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    d = dirs[:, :3].astype(np.float64)
    d = d[(d * d).sum(1) > 0]
    d /= np.linalg.norm(d, axis=1)[:, None]
    return float(np.degrees(np.arccos(np.clip(np.abs(v @ d.T).max(1), 0.0, 1.0))).max())


def scrambled(normal, K, seed):
    """A normal array with some words made -1, some made K (no direction of the table) and some made another direction."""
    rng = np.random.default_rng(seed)
    out = normal.copy()
    r = rng.random(len(out))
    out[r < 0.15] = -1
    out[(r >= 0.15) & (r < 0.25)] = K
    pick = (r >= 0.25) & (r < 0.5)
    out[pick] = rng.integers(0, K, int(pick.sum()))
    return out.astype(np.int32)


@functools.lru_cache(maxsize=None)
def street():
    """(the call that inserts the world, frame float64 [6000,3] in the sensor's axes, the true pose): a street of 20 m x 8 m at 0.2 m cells -
    a ground plane, two walls along it, and three car-sized boxes, the only evidence along the street - sampled densely for the map, and
    6000 rows drawn afresh from the same surfaces for the frame."""
    def surfaces(rng, count):
        share = rng.random(count)
        out = np.zeros((count, 3))
        g, wl, wr = share < 0.5, (share >= 0.5) & (share < 0.65), (share >= 0.65) & (share < 0.8)
        out[g] = np.stack([rng.uniform(0.3, 19.7, g.sum()), rng.uniform(-3.4, 3.4, g.sum()), rng.uniform(0.0, 0.02, g.sum())], -1)
        for mask, y in ((wl, -3.5), (wr, 3.5)):
            out[mask] = np.stack([rng.uniform(0.3, 19.7, mask.sum()), y + rng.uniform(-0.01, 0.01, mask.sum()), rng.uniform(0.0, 2.9, mask.sum())], -1)
        rest = np.flatnonzero(share >= 0.8)
        boxes = ((4.0, -2.0), (9.5, 1.5), (15.0, -1.0))  # corners; 2.0 x 1.2 x 1.4 m each
        which = rng.integers(0, 3, len(rest))
        face = rng.integers(0, 5, len(rest))
        u, v = rng.random(len(rest)), rng.random(len(rest))
        for j, i in enumerate(rest):
            x0, y0 = boxes[which[j]]
            f = face[j]
            if f == 0:
                out[i] = (x0 + 2.0 * u[j], y0 + 1.2 * v[j], 1.4)
            elif f in (1, 2):
                out[i] = (x0 + (2.0 if f == 2 else 0.0), y0 + 1.2 * u[j], 1.4 * v[j])
            else:
                out[i] = (x0 + 2.0 * u[j], y0 + (1.2 if f == 4 else 0.0), 1.4 * v[j])
        return out
    world = surfaces(np.random.default_rng(11), 120000)
    truth = np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 10.0, 0.3, 1.2])
    pts = surfaces(np.random.default_rng(12), 6000)
    frame = pts - truth[9:]
    world.setflags(write=False)
    frame.setflags(write=False)
    return cases.one_frame(world), frame, truth


def street_start(truth, degrees=0.5, shift=(0.09, -0.09, 0.085)):
    """The true pose turned by `degrees` about the axis (1, 1, 1) and shifted by `shift`: 0.5 degrees and 0.153 m off."""
    a = np.radians(degrees) * np.ones(3) / np.sqrt(3.0)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.linalg.norm(a)
    R = np.eye(3) + np.sin(t) / t * K + (1.0 - np.cos(t)) / (t * t) * (K @ K)
    return np.concatenate([(R @ truth[:9].reshape(3, 3)).reshape(9), truth[9:] + np.asarray(shift)])
