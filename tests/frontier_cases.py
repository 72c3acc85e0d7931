"""Masks and maps for tests/test_frontiers.py, painted cell by cell.  Every cluster case names a layout - how many components, which tile
seams their links cross - and realises() checks that on the CPU, with a flood fill of its own, before a GPU sees the case."""
import numpy as np

TILE = 64  # the side of a tile of the labelling kernel

# ---------------------------------------------------------------------------------------------------------------- the hand case

_F, _O, _U, _N = 0, 1, 2, 3  # free, occupied, seen but undecided, never seen
HAND_CELLS = [
    [_F, _F, _F, _F, _F, _F, _O, _N],   # (0,7): unknown, but its two neighbours inside the map are occupied - no frontier
    [_F, _N, _F, _F, _F, _F, _F, _O],   # (1,1): one unknown cell - its four neighbours link by diagonals only
    [_F, _F, _F, _F, _F, _F, _F, _F],
    [_F, _F, _F, _F, _F, _F, _F, _F],
    [_F, _F, _F, _F, _F, _F, _F, _F],   # (4,0..5) lie above unknown cells; pen blocks (4,2)
    [_U, _U, _N, _N, _U, _U, _F, _F],   # (5,6) touches (5,5); (5,7) touches only the map's edge - no frontier
]
HAND_OCCUPIED, HAND_FREE = 85, -40
HAND_BLOCKED = (4, 2)
HAND_MASK = [
    [0, 1, 0, 0, 0, 0, 0, 0],
    [1, 0, 1, 0, 0, 0, 0, 0],
    [0, 1, 0, 0, 0, 0, 0, 0],
    [0, 0, 0, 0, 0, 0, 0, 0],
    [1, 1, 0, 1, 1, 1, 0, 0],   # without pen (4,2) is a frontier cell too
    [0, 0, 0, 0, 0, 0, 1, 0],
]
_A, _B, _C = 1, 32, 35  # least linear indices: (0,1), (4,0), (4,3)
HAND_LABEL = [
    [-1, _A, -1, -1, -1, -1, -1, -1],
    [_A, -1, _A, -1, -1, -1, -1, -1],
    [-1, _A, -1, -1, -1, -1, -1, -1],
    [-1, -1, -1, -1, -1, -1, -1, -1],
    [_B, _B, -1, _C, _C, _C, -1, -1],
    [-1, -1, -1, -1, -1, -1, _C, -1],   # (4,5) - (5,6): a diagonal link
]
# (label, size, rep_r, rep_c, r0, c0, r1, c1).  The diamond's centroid cell (1,1) is no member and all four members are one cell away:
# the tie goes to the least index, (0,1).  B: sum_c = 1, cc = (2 + 2) // 4 = 1.  C: cr = (34 + 4) // 8 = 4, cc = (36 + 4) // 8 = 5.
HAND_ROWS = [[_A, 4, 0, 1, 0, 0, 2, 2], [_B, 2, 4, 1, 4, 0, 4, 1], [_C, 4, 4, 5, 4, 3, 5, 6], [-1] * 8]
HAND_SUMS = [[4, 4], [8, 1], [17, 18], [0, 0]]
HAND_INFO = [3, 3, 10, 3]


def hand_map():
    """-> (logodds int16 [6,8], last_seen int32 [6,8], pen uint8 [6,8])."""
    kind = np.array(HAND_CELLS)
    logodds = np.choose(kind, [HAND_FREE, HAND_OCCUPIED, HAND_FREE + 1, HAND_FREE - 60]).astype(np.int16)  # a never-seen cell's log-odds do not count
    last_seen = np.where(kind == _N, -1, 3).astype(np.int32)
    pen = np.zeros(kind.shape, np.uint8)
    pen[HAND_BLOCKED] = 255
    pen[0, 0] = 254  # the largest penalty of a free cell blocks nothing
    return logodds, last_seen, pen


# ---------------------------------------------------------------------------------------------------------------- flood fill

def components(mask):
    """int32, the shape of mask: -1 on zero bytes, elsewhere the least linear index of the cell's 8-connected component - by a flood fill
    in scan order, so the seed of a component is its least index."""
    M = np.asarray(mask) != 0
    rows, cols = M.shape
    label = np.full((rows, cols), -1, np.int32)
    for r0, c0 in zip(*np.nonzero(M)):
        if label[r0, c0] >= 0:
            continue
        seed, stack = int(r0) * cols + int(c0), [(int(r0), int(c0))]
        label[r0, c0] = seed
        while stack:
            r, c = stack.pop()
            for rr in range(max(0, r - 1), min(rows, r + 2)):
                for cc in range(max(0, c - 1), min(cols, c + 2)):
                    if M[rr, cc] and label[rr, cc] < 0:
                        label[rr, cc] = seed
                        stack.append((rr, cc))
    return label


def crossings(mask):
    """The kinds of tile seams that links between members cross: "h" (the tiles differ in their row only), "v" (in their column only),
    "d" (in both: over a four-tile corner)."""
    M = np.asarray(mask) != 0
    rows, cols = M.shape
    kinds = set()
    for dr, dc in ((0, 1), (1, -1), (1, 0), (1, 1)):
        for r, c in zip(*np.nonzero(M)):
            rr, cc = r + dr, c + dc
            if 0 <= rr < rows and 0 <= cc < cols and M[rr, cc]:
                dy, dx = r // TILE != rr // TILE, c // TILE != cc // TILE
                if dy or dx:
                    kinds.add("d" if dy and dx else "h" if dy else "v")
    return kinds


def tiles_with_members(mask):
    M = np.asarray(mask) != 0
    return len({(r // TILE, c // TILE) for r, c in zip(*np.nonzero(M))})


def realises(mask, n_components, kinds, label=None):
    """Does the mask hold n_components components whose links cross exactly the seams of `kinds`?  -> its labels."""
    got = components(mask) if label is None else label
    n = len(np.unique(got[got >= 0]))
    assert n == n_components, (n, n_components)
    assert crossings(mask) == set(kinds), (crossings(mask), kinds)
    return got


# ---------------------------------------------------------------------------------------------------------------- cluster cases

CLUSTER_SHAPES = [(1, 1), (1, 130), (130, 1), (64, 64), (65, 65), (63, 129), (129, 130), (192, 192)]


def _blank(shape):
    return np.zeros(shape, np.uint8)


def _paint(shape, cells, value=1):
    m = _blank(shape)
    for r, c in cells:
        m[r, c] = value
    return m


def _serpentine(shape):
    """One cell wide: every even row in full, joined to the next one at alternating ends."""
    rows, cols = shape
    m = _blank(shape)
    m[0::2] = 1
    for k, r in enumerate(range(1, rows - 1, 2)):
        m[r, cols - 1 if k % 2 == 0 else 0] = 1
    return m


def cluster_cases():
    """[(name, mask uint8, label int32)]: every layout on the smallest map that holds it, each checked against what its name says."""
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, mask, n, kinds):
        out.append((name, mask, realises(mask, n, kinds)))

    for shape in CLUSTER_SHAPES:
        tag = "%dx%d" % shape
        rows, cols = shape
        seams = {k for k, on in (("h", rows > TILE), ("v", cols > TILE), ("d", rows > TILE and cols > TILE)) if on}
        add("empty-" + tag, _blank(shape), 0, ())
        add("full-" + tag, np.full(shape, 7, np.uint8), 1, seams)  # any non-zero byte is a member
        half = (rng.random(shape) < 0.5).astype(np.uint8) * rng.integers(1, 256, shape, dtype=np.uint8)
        out.append(("random-" + tag, half, components(half)))
        if min(shape) > 1:
            add("checkerboard-" + tag, ((np.add.outer(np.arange(rows), np.arange(cols)) % 2) == 0).astype(np.uint8), 1, seams)  # every link a diagonal
    big = (129, 130)
    add("tile-corners", _paint(big, [(64, 64), (64, 127), (127, 64), (127, 127)]), 4, ())
    add("map-corners", _paint(big, [(0, 0), (0, 129), (128, 0), (128, 129)]), 4, ())
    add("pair-over-a-horizontal-seam", _paint(big, [(63, 10), (64, 10)]), 1, "h")
    add("pair-over-a-horizontal-seam-slanted", _paint(big, [(63, 70), (64, 71), (63, 90), (64, 89)]), 2, "h")
    add("pair-over-a-vertical-seam", _paint(big, [(10, 63), (10, 64)]), 1, "v")
    add("pair-over-a-vertical-seam-slanted", _paint(big, [(70, 63), (71, 64), (90, 64), (91, 63)]), 2, "v")
    for shape in ((65, 65), big):
        add("corner-diagonal-%dx%d" % shape, _paint(shape, [(63, 63), (64, 64)]), 1, "d")
        add("corner-antidiagonal-%dx%d" % shape, _paint(shape, [(63, 64), (64, 63)]), 1, "d")
    add("both-corner-diagonals", _paint(big, [(63, 63), (64, 64), (63, 64), (64, 63)]), 1, "hvd")
    add("last-column-of-a-tile-to-the-tile-below", _paint(big, [(63, 0), (64, 1), (63, 127), (64, 128), (63, 129), (64, 128)]), 2, "hd")

    # a U: two arms in tile (0,0) that join only through tile (0,1) - two tile-local roots of one tile become one label
    u = _paint(big, [(10, c) for c in range(50, 64)] + [(20, c) for c in range(50, 64)] + [(r, 64) for r in range(10, 21)])
    assert len(np.unique(components(u[:TILE, :TILE])[u[:TILE, :TILE] != 0])) == 2
    add("u-through-the-neighbour-tile", u, 1, "v")

    # the least index lies in tile (0,2), the far end of a path (0,2) -> (1,2) -> (1,1) -> (1,0) -> (0,0)
    path = [(r, 129) for r in range(5, 101)] + [(100, c) for c in range(2, 130)] + [(r, 2) for r in range(20, 101)]
    far = _paint(big, path)
    label = realises(far, 1, "hv")
    assert label[20, 2] == 5 * 130 + 129 and tiles_with_members(far) == 5
    out.append(("least-index-in-the-last-tile-reached", far, label))

    # a comb in the second tile row: its spine crosses both vertical seams, the teeth stand on odd columns - a tile-local root is the
    # top of the tile's first tooth, off the tile's first row and first column
    comb = _paint(big, [(70, c) for c in range(5, 126)] + [(r, c) for c in range(5, 126, 2) for r in range(66, 70)])
    label = realises(comb, 1, "v")
    for tx in range(2):  # the comb ends before the third tile
        piece = comb[TILE:2 * TILE, tx * TILE:(tx + 1) * TILE]
        r, c = (int(v[0]) for v in np.nonzero(piece))
        assert r > 0 and c > 0, (tx, r, c)
    out.append(("comb-with-roots-off-the-seams", comb, label))

    snake = _serpentine((192, 192))
    label = realises(snake, 1, "hv")
    assert tiles_with_members(snake) == 9 and int(snake.sum()) == 96 * 192 + 95
    out.append(("serpentine-through-nine-tiles", snake, label))
    return out


def inside_tiles_mask():
    """192 x 192: random members, none on the first row or first column of a tile - no link crosses a seam - and tile (1,1) empty.
    -> (mask, the number of tiles with a member)."""
    rng = np.random.default_rng(7)
    m = (rng.random((192, 192)) < 0.5).astype(np.uint8)
    m[0::TILE] = 0
    m[:, 0::TILE] = 0
    m[TILE:2 * TILE, TILE:2 * TILE] = 0
    assert crossings(m) == set() and tiles_with_members(m) == 8
    return m, 8


# ---------------------------------------------------------------------------------------------------------------- cells cases

# 67 x 131 cells are more than one workgroup's span; 3 x 4100 and 2 x 4096 stand on either side of the row length up to which the rows
# above and below are staged
CELLS_SHAPES = [(1, 1), (1, 17), (17, 1), (67, 131), (2, 4096), (3, 4100)]
CELLS_LOGODDS = (-100, -41, -40, -39, 0, 84, 85, 86, 300)
CELLS_THRESHOLDS = [(occupied, free) for occupied in (84, 85, 86) for free in (-41, -40, -39)]


def cells_map(shape, seed):
    """Random (logodds int16, last_seen int32, pen uint8): a third of the cells never seen, a quarter of pen blocked."""
    rng = np.random.default_rng(seed)
    logodds = rng.choice(np.array(CELLS_LOGODDS, np.int16), shape)
    last_seen = rng.choice(np.array([-1, 0, 9], np.int32), shape)
    pen = rng.choice(np.array([0, 17, 254, 255], np.uint8), shape)
    return logodds, last_seen, pen
