"""Inputs for a frame aligned to the voxel map (group (X)).  The maps come from voxel_map_cases and voxel_match_cases; the independent model
is stereo_vision.sv.voxel_map_align_sums_brute, one Python loop per row over all voxels."""
import math

import numpy as np

import voxel_map_cases as cases
import voxel_match_cases as mcases
from voxel_map_cases import BOX16, IDENTITY
from voxel_match_cases import shifted

FIELDS = ("sums", "pair_key", "pair_d2")
DTYPES = dict(sums=np.int64, pair_key=np.int64, pair_d2=np.int32)
MAX_DISTS = (0.0, 0.5, 1.0, 2.0)
HAND = dict(lo=(0.0, 0.0, -0.9), hi=(4.0, 4.0, 1.1), size=1.0, capacity=512)  # test_voxel_match's: 4 x 4 x 2 cells
LONG_BOX = dict(lo=(0.0, 0.0, 0.0), hi=(1048576.0, 4.0, 4.0), size=1.0, capacity=512)  # 2^20 cells on x: a cell one too high carries into y


def same(got, want, fields=FIELDS):
    """Shape, dtype and bits of every field."""
    for k in fields:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if a.shape != b.shape or a.dtype != b.dtype or a.dtype != DTYPES[k] or a.tobytes() != b.tobytes():
            return False
    return True


def define(sv, params, calls):
    state, seq = sv.voxel_map_state(sv.voxel_map_params(**params)), 0
    for call in calls:
        sv.voxel_map_insert(state, *call, seq0=seq)
        seq += call[0].shape[0]
    return state


def key_of(cell):
    return int(cell[0]) | int(cell[1]) << 20 | int(cell[2]) << 40


def hand_calls():
    """test_voxel_match's hand map - voxel a = cell (1, 2, 0) with mean offsets (32768, 0, 32768), voxel b = cell (1, 2, 1) with (32768,
    16384, 65535) - and one call more: voxel c = cell (3, 2, 0) with a's offsets, which a row can be as far from as from a."""
    top = math.nextafter(1.1, 0.0)
    f0 = np.array([[2.0, -1.5, -0.4], [np.nan, 1.0, 0.0], [1.0, 0.0, -0.4]])
    f1 = np.array([[0.5, 2.25, top - 0.5], [0.5, 2.0, -0.9], [9.0, 9.0, 9.0]])
    n = np.array([[3, 1, 1], [5, 2, 1]], np.int32)
    return [(np.stack([f0, f1]), None, n, np.array([3, 2], np.int32), np.stack([cases.QUARTER, shifted((1.0, 0.0, 0.5))])),
            cases.one_frame(np.array([[3.5, 2.0, -0.4]]))]


def hand_frame():
    """(xyz, n, counts): six rows under the identity.  In 1/256 of a cell: a stands at (384, 512, 128), b at (384, 576, 511), c at (896,
    512, 128)."""
    top = math.nextafter(1.1, 0.0)  # t = 2.0: the cell is clamped to 1 and u to 65535
    xyz = np.array([[[1.5, 2.0, -0.4],    # p = (384, 512, 128): on a's mean
                     [2.5, 2.0, -0.4],    # p = (640, 512, 128) in the empty cell (2, 2, 0): 256 from a and from c on x alone
                     [0.25, 1.25, -0.4],  # p = (64, 320, 128) in cell (0, 1, 0): a is the nearest, 320^2 + 192^2 = 139264 away
                     [1.5, 2.0, -0.4],    # weight 0
                     [np.nan, 2.0, -0.4],
                     [1.25, 2.5, top]]])  # p = (320, 640, 511) in b's cell: 64^2 + 64^2 = 8192 from b
    return xyz, np.array([[1, 3, 5, 0, 7, 2]], np.int32), np.array([6], np.int32)


def random_align(seed):
    """(params, calls, (xyz, n, counts), poses [4][3,12], origin, max_dist, filters): voxel_map_cases.random_case(seed) as the map; frame 0
    of its call three times as the frames to align - one with its own count, one with a count of 0 or -1, one with a count above cap -
    at four poses each: the frame's own, a fraction of a cell off, a cell off, and a pose with a word that is not finite."""
    params, calls = cases.random_case(seed)
    xyz, _, n, counts, poses = calls[0]
    size, cap = params["size"], xyz.shape[1]
    frames = (np.stack([xyz[0]] * 3), None if n is None else np.stack([n[0]] * 3), np.array([max(int(counts[0]), cap // 2), -(seed % 2), cap + 7], np.int32))
    bad = shifted((0.0, 0.0, 0.0))
    bad[seed % 12] = (np.nan, np.inf)[seed % 2]
    variants = [poses[0], shifted((0.3 * size, -0.45 * size, 0.2 * size), poses[0]), shifted((size, 0.0, -size), poses[0]), bad]
    rng = np.random.default_rng(seed)
    origin = rng.integers(-5000, 5000, (3, 3)).astype(np.int32)
    filters = (dict(), dict(min_rows=2), dict(min_n=3, since=0))[seed % 3]
    return params, calls, frames, [np.stack([p] * 3) for p in variants], origin, MAX_DISTS[seed % 4], filters


def edge_case():
    """(params, calls, (xyz, n, counts)) in BOX16: voxels in a cell of each of the six faces and in two opposite corners, and rows in every
    cell of the box within one cell of one of them."""
    rng = np.random.default_rng(77)
    at = np.array([(0, 5, 5), (15, 5, 5), (5, 0, 5), (5, 15, 5), (5, 5, 0), (5, 5, 15), (0, 0, 0), (15, 15, 15)])
    voxels = np.concatenate([at, np.clip(at + rng.integers(-1, 2, at.shape), 0, 15)])
    calls = [cases.one_frame(voxels + rng.uniform(0.05, 0.95, voxels.shape), None, rng.integers(1, 9, len(voxels)))]
    around = np.array([(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)])
    cells = (at[:, None, :] + around[None]).reshape(-1, 3)
    cells = cells[((cells >= 0) & (cells < 16)).all(1)]
    rows = cells + rng.uniform(0.0, 1.0, cells.shape)
    return BOX16, calls, (rows[None], None, np.array([len(rows)], np.int32))


def long_case():
    """(params, calls, (xyz, n, counts)) in LONG_BOX: a voxel in cell (0, 1, 0), whose key 1 << 20 is what cell (2^20, 0, 0) would shift
    to, one in cell (2^20 - 2, 0, 0), and rows in the last cells of x."""
    calls = [cases.one_frame(np.array([[0.5, 1.5, 0.5], [1048574.5, 0.5, 0.5]]))]
    rows = np.array([[1048575.5, 0.5, 0.5], [1048575.25, 0.75, 0.25], [1048574.5, 1.5, 0.5], [0.5, 0.5, 0.5]])
    return LONG_BOX, calls, (rows[None], None, np.array([len(rows)], np.int32))


def tombstone_case():
    """(params, calls, carve, (xyz, n, counts)): BOX16 with voxels in cells (5, 5, 5) and (6, 5, 5) at offset 0.5; the carve's one ray runs
    along y through (5, 5, 5) alone.  The frame's row stands on the mean of the voxel that is emptied."""
    calls = [cases.one_frame(cases.cell_points([(5, 5, 5), (6, 5, 5)]))]
    carve = dict(xyz=np.array([[[5.5, 9.5, 5.5]]]), n=None, counts=np.array([1], np.int32), poses=IDENTITY[None], origin=(5.5, 2.5, 5.5), seq0=1)
    return BOX16, calls, carve, (np.array([[[5.5, 5.5, 5.5]]]), None, np.array([1], np.int32))


def rotation(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    return rz @ ry @ rx


def scene_truth(sv):
    x, y, z, yaw = mcases.SCENE_TRUTH
    return sv.voxel_map_pose(x, y, yaw, z)


def scene_start(sv, roll, pitch, yaw, shift):
    """The scene's true pose composed with a rotation and shifted."""
    truth = scene_truth(sv)
    return np.concatenate([(rotation(roll, pitch, yaw) @ truth[:9].reshape(3, 3)).reshape(9), truth[9:] + np.asarray(shift, np.float64)])


def pose_error(pose, truth):
    """(degrees, metres) between two poses."""
    r = pose[:9].reshape(3, 3) @ truth[:9].reshape(3, 3).T
    return math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(r) - 1.0) / 2.0)))), float(np.linalg.norm(pose[9:] - truth[9:]))


SCENE_STARTS = {"all": (0.017, -0.026, 0.035, (0.10, -0.08, 0.06)), "yaw": (0.0, 0.0, 0.035, (0.10, -0.08, 0.06))}


def scene_case(dtype=np.float64):
    """(the call that inserts the world, (xyz, n, counts) of the 600-point frame)."""
    world, frame = mcases.scene()
    return cases.one_frame(world.copy(), None, None, IDENTITY, np.float64), (frame.astype(dtype)[None], None, np.array([len(frame)], np.int32))
