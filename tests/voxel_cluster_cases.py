"""Inputs for the connected components of the voxel map (group (W)).  A case is a dict: params (the voxel map's), ops - a list of
("update", call) and ("carve", call, keywords) steps, a call as voxel_map_cases has it -, spec (the eight words of the clustering), flat
(None, or the flat map's words and the flatten's words for mode 1: the floor is the flatten's) and kw (min_n, min_rows, since).  Every map
but the wrap's is BOX16-like with a table of 1024 slots, and each case is there because one mistake shows on it."""
import numpy as np

from voxel_flatten_cases import flat_words
from voxel_flatten_cases import words as flatten_words
from voxel_map_cases import BOX16, PROBE_BOX, cell_points, colliding_cells, one_frame

OPEN = 2 ** 30


def words(connectivity=26, mode=0, z_ref_q=0, h_lo_q=-OPEN, h_hi_q=OPEN, min_voxels=1, capacity=1024, drop=0):
    return dict(connectivity=connectivity, mode=mode, z_ref_q=z_ref_q, h_lo_q=h_lo_q, h_hi_q=h_hi_q, min_voxels=min_voxels, capacity=capacity, drop=drop)


def case(params, ops, spec, flat=None, **kw):
    return dict(params=params, ops=ops, spec=spec, flat=flat, kw=kw)


def updates(*cell_lists, **frame):
    return [("update", one_frame(cell_points(cells), **frame)) for cells in cell_lists]


def cube(x, y, z, side=2):
    return [(x + i, y + j, z + k) for i in range(side) for j in range(side) for k in range(side)]


TOUCH = {"face": (4, 2, 2), "edge": (4, 4, 2), "corner": (4, 4, 4)}                 # where the second cube of 2 x 2 x 2 starts; the first starts at (2, 2, 2)
TOUCH_COMPONENTS = {"face": (1, 1, 1), "edge": (2, 1, 1), "corner": (2, 2, 1)}  # at connectivity 6, 18, 26


def touch_cases():
    return {"touch_%s_%d" % (how, conn): case(BOX16, updates(cube(2, 2, 2) + cube(*at)), words(connectivity=conn))
            for how, at in TOUCH.items() for conn in (6, 18, 26)}


WRAP_CELLS = 2 ** 20  # the most cells per axis a voxel map admits


def wrap_cases():
    """A box with 2^20 cells on one axis: key - 1 of the cell (0, 5, 5) is the key of (2^20 - 1, 4, 5), a voxel of the map, and no
    neighbour; likewise a step down axis 1 from (7, 0, 5) lands on (7, 2^20 - 1, 4).  And the two ends of a 16-cell axis."""
    n = WRAP_CELLS
    box_x = dict(lo=(0.0, 0.0, 0.0), hi=(float(n), 16.0, 16.0), size=1.0, capacity=512)
    box_y = dict(lo=(0.0, 0.0, 0.0), hi=(16.0, float(n), 16.0), size=1.0, capacity=512)
    return {"wrap_x": case(box_x, updates([(0, 5, 5), (n - 1, 4, 5), (8, 0, 9), (8, 15, 9), (9, 3, 0), (9, 3, 15)]), words()),
            "wrap_y": case(box_y, updates([(7, 0, 5), (7, n - 1, 4), (0, 8, 9), (15, 8, 9)]), words())}


LINE = [(4, 8, 8), (5, 8, 8), (6, 8, 8)]


def tombstone_cases():
    """A line of three voxels whose middle one is carved - a ray of a second frame along axis 1 through (5, 8, 8) - or is too light."""
    seen = one_frame(cell_points(LINE), n=[5, 1, 5])
    ray = one_frame(cell_points([(5, 14, 8)]))
    carve = ("carve", ray, dict(origin=(5.5, 2.5, 8.5), seq0=1, reach=20, margin=1, min_miss=1, ratio=0, apply=True))
    return {"tombstone_carved": case(BOX16, [("update", seen), carve], words()),
            "tombstone_min_n": case(BOX16, [("update", seen)], words(), min_n=2)}


PROBE_SLOT = 1022


def probe_case(slot_of):
    """Four cells whose keys start probing at slot 1022 - they lie at 1022, 1023, 0 and 1 - and the cell behind each on axis 0, which looks
    its neighbour up through the chain around the table's end."""
    held = colliding_cells(slot_of, PROBE_SLOT, 4)
    held = held[held[:, 0] < 63]
    behind = held + np.array([1, 0, 0])
    return case(PROBE_BOX, updates(held, behind), words(connectivity=6))


def schedule_cells():
    rng = np.random.default_rng(7)
    flat = rng.choice(16 * 16 * 6, 300, replace=False)  # 300 of the 1536 cells of six layers: many pieces, many collisions in 1024 slots
    return np.stack([flat % 16, (flat // 16) % 16, 5 + flat // 256], -1)


def schedule_cases():
    """The same voxels in one frame in three row orders, the third with idle rows behind its count: the table's layout follows the order,
    the result does not."""
    cells = schedule_cells()
    shuffled = cells[np.random.default_rng(8).permutation(len(cells))]
    padded = np.concatenate([shuffled, np.zeros((37, 3), np.int64)])
    return {"schedule_in_order": case(BOX16, updates(cells), words()), "schedule_reversed": case(BOX16, updates(cells[::-1]), words()),
            "schedule_shuffled": case(BOX16, updates(padded, count=len(cells)), words())}


def snake_path():
    """A 6-connected path through BOX16: rows of 16 cells at even y, joined at alternating ends through odd y, three such layers at even z
    joined through odd z.  407 cells."""
    path, x_up, y_up = [], True, True
    for z in (0, 2, 4):
        ys = list(range(0, 16, 2)) if y_up else list(range(14, -1, -2))
        for k, y in enumerate(ys):
            xs = range(16) if x_up else range(15, -1, -1)
            path += [(x, y, z) for x in xs]
            x_up = not x_up
            if k + 1 < len(ys):
                path.append((path[-1][0], (y + ys[k + 1]) // 2, z))
        y_up = not y_up
        if z < 4:
            path.append((path[-1][0], path[-1][1], z + 1))
    return path


def snake_cases():
    path = snake_path()
    return {"snake_forward": case(BOX16, updates(path), words(connectivity=6)), "snake_backward": case(BOX16, updates(path[::-1]), words(connectivity=6)),
            "snake_every_second": case(BOX16, updates(path[::2]), words(connectivity=6))}


def slab_case():
    """Two full layers: 512 voxels, the capacity, in one component - every wavefront adds to one root and one row."""
    return case(BOX16, updates([(x, y, z) for z in (3, 4) for y in range(16) for x in range(16)]), words(connectivity=6))


SIZES_K = 4
SIZES_LINES = {3: (1, 2, 2), 4: (1, 6, 2), 5: (1, 10, 2)}  # voxels: where the line along axis 0 starts


def sizes_cases():
    cells = [(x + i, y, z) for count, (x, y, z) in SIZES_LINES.items() for i in range(count)]
    frame = dict(n=np.arange(1, len(cells) + 1))
    return {"sizes_keep": case(BOX16, updates(cells, **frame), words(min_voxels=SIZES_K)), "sizes_drop": case(BOX16, updates(cells, **frame), words(min_voxels=SIZES_K, drop=1))}


CAPACITY_SINGLES, CAPACITY_ROWS = 70, 64


def capacity_case():
    i = np.arange(CAPACITY_SINGLES)
    cells = np.stack([2 * (i % 8), 2 * ((i // 8) % 8), 2 * (i // 64)], -1)
    order = np.random.default_rng(9).permutation(CAPACITY_SINGLES)
    return case(BOX16, updates(cells[order]), words(capacity=CAPACITY_ROWS))


FLOOR_FLAT = ((0, 14), (0, 16), 1)
FLOOR_POSTS, FLOOR_WALL, FLOOR_OUTSIDE = [(3, 3), (10, 4)], [(x, 12) for x in range(6, 10)], (15, 8)


def floor_cells():
    ground = [(x, y, 0) for x in range(16) for y in range(16)]
    posts = [(x, y, z) for x, y in FLOOR_POSTS for z in (1, 2, 3)]
    wall = [(x, y, z) for x, y in FLOOR_WALL for z in (1, 2)]
    outside = [FLOOR_OUTSIDE + (z,) for z in (1, 2)]  # a post beyond the flat map's last row
    return ground + posts + wall + outside


def floor_cases():
    """A ground plane with two posts and a wall on it: one piece over all heights, three over the flatten's floor."""
    flat = dict(map=flat_words(*FLOOR_FLAT), flatten=flatten_words(step_q=128, height_q=2048, radius=2))
    return {"floor_all_heights": case(BOX16, updates(floor_cells()), words()),
            "floor_over_the_floor": case(BOX16, updates(floor_cells()), words(mode=1, h_lo_q=128, h_hi_q=2048), flat=flat)}


def band_case():
    """Mode 0: a column of six voxels of which the band takes the middle two pairs apart: zq - z_ref_q one below, at and above the ends."""
    column = [(8, 8, z) for z in range(6)]  # zq = 128 + 256 z
    return case(BOX16, updates(column), words(z_ref_q=100, h_lo_q=284, h_hi_q=1052))  # h = 28, 284, 540, 796, 1052, 1308: z = 1, 2, 3


def all_cases(slot_of):
    """{name: case}; slot_of: stereo_vision.sv.voxel_map_slot_of."""
    cases = {"probe": probe_case(slot_of), "slab": slab_case(), "capacity": capacity_case(), "band": band_case(), "empty": case(BOX16, [], words()),
             "overflowed": case(dict(BOX16, capacity=1), updates([(4, 4, 4), (5, 4, 4)]), words())}
    for more in (touch_cases(), wrap_cases(), tombstone_cases(), schedule_cases(), snake_cases(), sizes_cases(), floor_cases()):
        cases.update(more)
    return cases
