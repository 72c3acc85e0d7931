"""Case builders for test_cost_to_goal.py: maps of penalties with their goals, small enough for the Dijkstra definition, at every size and
place where the sweep kernel's tiling of 64 x 64 cells can go wrong.  A case is (pen uint8 [rows, cols], goals int32 [G, 2])."""
import numpy as np

BLOCKED = 255
TILE = 64

HAND_PEN = np.zeros((5, 7), np.uint8)
HAND_PEN[1:4, 3] = BLOCKED
HAND_PEN[0, 5] = 20
HAND_GOALS = np.array([[2, 0]], np.int32)
I = 0x7FFFFFFF
HAND_COST = np.array([[20, 24, 28, 38, 48, 78, 76],
                      [10, 14, 24, I, 58, 62, 72],
                      [0, 10, 20, I, 68, 72, 76],
                      [10, 14, 24, I, 58, 62, 72],
                      [20, 24, 28, 38, 48, 58, 68]], np.int32)
# from (2, 6): both diagonals towards column 5 offer 62 + 14; (-1, -1) comes before (1, -1) in the order of the moves
HAND_ROUTE = [(2, 6), (1, 5), (0, 4), (0, 3), (0, 2), (1, 1), (2, 0)]


def random_map(rng, rows, cols, blocked, n_goals):
    """Penalties 0 .. 254, a share `blocked` of the cells blocked ("one": exactly one cell), goals anywhere from two cells outside the map
    inwards - so some fall outside and some on blocked cells."""
    pen = rng.integers(0, 255, (rows, cols)).astype(np.uint8)
    if blocked == "one":
        pen[rng.integers(0, rows), rng.integers(0, cols)] = BLOCKED
    else:
        pen[rng.random((rows, cols)) < blocked] = BLOCKED
    goals = np.stack([rng.integers(-2, rows + 2, n_goals), rng.integers(-2, cols + 2, n_goals)], -1).astype(np.int32)
    return pen, goals


def serpentine(n=130):
    """n x n: every odd row is a wall with one gap, at the right end and the left end in turn; the goal is (0, 0).  The only path runs
    along every even row and re-enters every tile of 64 x 64 cells many times: tiles go clean and dirty again."""
    pen = np.zeros((n, n), np.uint8)
    for k, r in enumerate(range(1, n, 2)):
        pen[r] = BLOCKED
        pen[r, n - 1 if k % 2 == 0 else 0] = 0
    return pen, np.array([[0, 0]], np.int32)


def tile_corner(blocked_cell, rows=70, cols=70, seed=3):
    """The four cells that meet at the corner of four tiles, (63, 63), (63, 64), (64, 63) and (64, 64): the goal on (63, 63) and one of the
    other three blocked, so that the diagonal across the corner is admitted or refused by cells of other tiles.  Light random penalties."""
    rng = np.random.default_rng(seed)
    pen = rng.integers(0, 4, (rows, cols)).astype(np.uint8)
    pen[TILE - 1:TILE + 1, TILE - 1:TILE + 1] = 0
    if blocked_cell is not None:
        pen[blocked_cell] = BLOCKED
    return pen, np.array([[TILE - 1, TILE - 1]], np.int32)


def field_cases():
    """name -> case: maps smaller than a tile, tile-edge sizes, goals at a tile's corners and across them, the corner rule across tiles,
    the largest sums, and fields without any finite cost."""
    rng = np.random.default_rng(41)
    cases = {"1x1": (np.zeros((1, 1), np.uint8), np.array([[0, 0]], np.int32)),
             "1x7": (np.array([[0, 3, 0, BLOCKED, 0, 9, 0]], np.uint8), np.array([[0, 1], [0, 6]], np.int32)),
             "hand": (HAND_PEN, HAND_GOALS)}
    for rows, cols in ((64, 64), (65, 65), (64, 129), (130, 130)):
        pen, _ = random_map(rng, rows, cols, 0.2, 1)
        corners = [(0, 0), (0, min(cols, TILE) - 1), (min(rows, TILE) - 1, 0), (TILE - 1, TILE - 1), (TILE, TILE), (TILE - 1, TILE)]
        for k, g in enumerate(corners):
            if g[0] < rows and g[1] < cols:
                p = pen.copy()
                p[g] = 0
                cases["%dx%d goal %d,%d" % (rows, cols, g[0], g[1])] = (p, np.array([g], np.int32))
        cases["%dx%d three goals" % (rows, cols)] = random_map(rng, rows, cols, 0.3, 3)
    for name, cell in (("free", None), ("63,64", (TILE - 1, TILE)), ("64,63", (TILE, TILE - 1)), ("64,64", (TILE, TILE))):
        cases["corner %s" % name] = tile_corner(cell)
    cases["pen 254"] = (np.full((65, 65), 254, np.uint8), np.array([[0, 0]], np.int32))
    cases["all blocked"] = (np.full((65, 70), BLOCKED, np.uint8), np.array([[3, 3], [64, 69]], np.int32))
    no_goal = random_map(rng, 65, 70, 0.2, 1)[0]
    no_goal[5, 5] = BLOCKED
    cases["no valid goal"] = (no_goal, np.array([[5, 5], [-1, 3], [65, 0], [0, 70]], np.int32))
    return cases


def stuck_field():
    """A hand-made field that is no fixed point: from (0, 0) the walk goes downhill to (0, 2), whose neighbours all cost more - status 4
    with three cells kept."""
    pen = np.zeros((3, 5), np.uint8)
    cost = np.array([[50, 40, 30, 60, 0],
                     [70, 70, 70, 70, 70],
                     [80, 80, 80, 80, 80]], np.int32)
    return cost, pen, [(0, 0), (0, 1), (0, 2)]
