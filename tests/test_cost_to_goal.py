"""Group (N): the penalties made from the clearance field, the cost-to-goal field of the world map and the routes traced through it -
stereo_vision.sv.cost_cells / cost_to_goal / cost_to_goal_relax / cost_routes, the C entries sv_cost_*, engine.cost_cells /
occupancy_cost_to_goal / cost_routes and rig.OccupancyMap.cost_to_goal / routes.

Every comparison is exact - shape, dtype and bits: all arithmetic is integer, and a shortest-path length under strictly positive weights
is unique, so any relaxation order that reaches a fixed point from the all-COST_INF start gives the same bits as Dijkstra's algorithm.
A route is a deterministic walk over such a field with a stated tie order."""
import ctypes
import os
import re

import numpy as np
import pytest

import cost_cases
import util
from cost_cases import BLOCKED, HAND_COST, HAND_GOALS, HAND_PEN, HAND_ROUTE
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_occupancy_map import CLI_GRID, _drive_frames, drive  # noqa: F401 (drive: the committed KITTI frames' states, a fixture)
from test_clearance import _fused_recovery_maps
from test_map_match import RECOVERY_FRAME

SV_ERR_ARG = -1
INF = 0x7FFFFFFF
ROUTE_KEYS = ("cells", "length", "status")


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.fixture(scope="module")
def fields(sv):
    """name -> (pen, goals, Dijkstra's field): every reference of the GPU tests, computed once and never changed."""
    out = {name: (pen, goals, sv.cost_to_goal(pen, goals)) for name, (pen, goals) in cost_cases.field_cases().items()}
    pen, goals = cost_cases.serpentine()
    out["serpentine"] = (pen, goals, sv.cost_to_goal(pen, goals))
    for _, _, want in out.values():
        want.setflags(write=False)  # _cuda copies what it uploads
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_hand_case_in_both_forms(sv):
    for form in (sv.cost_to_goal, sv.cost_to_goal_relax):
        got = form(HAND_PEN, HAND_GOALS)
        assert _bits(got, HAND_COST)
        assert got[1, 4] == 58  # not 52: the diagonal from (0, 3) would cut the wall's corner
        assert got[0, 5] == 78 and got[0, 6] == 76  # (0, 5) pays its 20; (0, 6) goes round it through (1, 5)
    assert sv.COST_INF == INF and sv.COST_BLOCKED == 255


def test_dijkstra_equals_relaxation(sv):
    rng = np.random.default_rng(7)
    shares = (0, "one", 0.1, 0.45, 1)
    n, ignored = 0, 0
    for k in range(35):
        rows, cols = (int(v) for v in rng.integers(1, 41, 2))
        pen, goals = cost_cases.random_map(rng, rows, cols, shares[k % 5], 1 + k % 3)
        a, b = sv.cost_to_goal(pen, goals), sv.cost_to_goal_relax(pen, goals)
        assert _bits(a, b) and a.dtype == np.int32, (k, rows, cols)
        inside = (goals[:, 0] >= 0) & (goals[:, 0] < rows) & (goals[:, 1] >= 0) & (goals[:, 1] < cols)
        ignored += int((~inside).sum()) + int((pen[goals[inside, 0], goals[inside, 1]] == BLOCKED).sum())
        assert ((a == INF) | (pen != BLOCKED)).all()
        n += 1
    assert n >= 30 and ignored > 5


def test_corner_rule_and_ignored_goals(sv):
    # a pocket walled in diagonally: (0, 0) touches the rest of the map only across the corner between (0, 1) and (1, 0)
    pen = np.zeros((4, 4), np.uint8)
    pen[0, 1] = pen[1, 0] = BLOCKED
    out = sv.cost_to_goal(pen, [(3, 3)])
    assert out[0, 0] == INF and out[1, 1] == 28 and _bits(out, sv.cost_to_goal_relax(pen, [(3, 3)]))
    back = sv.cost_to_goal(pen, [(0, 0)])  # and from the inside: nothing leaves the pocket
    assert back[0, 0] == 0 and (back.ravel()[1:] == INF).all() and _bits(back, sv.cost_to_goal_relax(pen, [(0, 0)]))
    # a goal on a blocked cell is ignored; with no valid goal everything is COST_INF
    both = sv.cost_to_goal(pen, [(0, 1), (3, 3)])
    assert _bits(both, out)
    for form in (sv.cost_to_goal, sv.cost_to_goal_relax):
        assert (form(pen, [(0, 1), (-1, 0), (4, 0), (0, 4)]) == INF).all()
        assert (form(np.full((3, 3), BLOCKED, np.uint8), [(1, 1)]) == INF).all()


def test_cost_cells(sv):
    v = np.arange(65536)
    assert np.array_equal(sv.cost_isqrt(v), np.floor(np.sqrt(v.astype(np.float64))).astype(np.int64))  # exact below 2^52
    root = sv.cost_isqrt(v)
    assert (root * root <= v).all() and ((root + 1) * (root + 1) > v).all()  # and by the root's own definition
    d2 = np.array([[0, 8, 9, 10, 15, 16, 17, 99, 100, 65535]], np.uint16)
    pen = sv.cost_cells(d2, 9, soft=10, weight=3, radius=10)
    assert pen.dtype == np.uint8 and pen.tolist() == [[255, 255, 255, 21, 21, 18, 18, 3, 0, 0]]  # d2 == r2_block blocks; 65535 gives 0
    assert sv.cost_cells(d2, 0, radius=10).tolist() == [[255, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
    assert sv.cost_cells(d2, 0, soft=254, weight=254, radius=10).tolist() == [[255] + [254] * 8 + [0]]  # the weight saturates at 254
    assert sv.cost_cells(d2, 100, radius=10)[0, 8] == 255
    for bad in (dict(r2_block=101), dict(r2_block=-1), dict(soft=255), dict(weight=255), dict(weight=-1), dict(soft=1.5), dict(radius=0), dict(radius=255),
                dict(d2=d2.astype(np.int32)), dict(d2=d2[0])):
        with pytest.raises(ValueError):
            sv.cost_cells(**dict(dict(d2=d2, r2_block=9, soft=1, weight=1, radius=10), **bad))


def test_routes(sv):
    got = sv.cost_routes(HAND_COST, HAND_PEN, [(2, 6)], 10)
    assert got["cells"].dtype == np.int16 and got["cells"].shape == (1, 10, 2) and got["length"].dtype == got["status"].dtype == np.int32
    assert got["cells"][0, :7].tolist() == [list(c) for c in HAND_ROUTE] and (got["cells"][0, 7:] == -1).all()
    assert got["length"].tolist() == [7] and got["status"].tolist() == [0]
    # a tie resolved by the stated order: from the centre of a symmetric field every axial neighbour offers the same; (-1, 0) is first
    pen = np.zeros((3, 3), np.uint8)
    ring = sv.cost_to_goal(pen, [(0, 1), (1, 0), (1, 2), (2, 1)])
    assert ring[1, 1] == 10 and sv.cost_routes(ring, pen, [(1, 1)], 5)["cells"][0, :2].tolist() == [[1, 1], [0, 1]]
    diag = sv.cost_to_goal(pen, [(0, 0), (0, 2), (2, 0), (2, 2)])  # axial 10 + 10 against diagonal 0 + 14: the first diagonal
    assert sv.cost_routes(diag, pen, [(1, 1)], 5)["cells"][0, :2].tolist() == [[1, 1], [0, 0]]
    # statuses 1 and 2 with length 0, a goal as its own route, and 3 at exactly capacity
    got = sv.cost_routes(HAND_COST, HAND_PEN, [(-1, 0), (5, 0), (0, 7), (1, 3), (2, 0), (2, 6), (2, 6)], 7)
    assert got["status"].tolist() == [1, 1, 1, 2, 0, 0, 0] and got["length"].tolist() == [0, 0, 0, 0, 1, 7, 7] and (got["cells"][:4] == -1).all()
    got = sv.cost_routes(HAND_COST, HAND_PEN, [(2, 6)], 6)
    assert got["status"].tolist() == [3] and got["length"].tolist() == [6] and got["cells"][0].tolist() == [list(c) for c in HAND_ROUTE[:6]]
    assert sv.cost_routes(HAND_COST, HAND_PEN, [(2, 6)], 1)["status"].tolist() == [3]
    unreachable = sv.cost_to_goal(np.array([[0, BLOCKED, 0]], np.uint8), [(0, 0)])
    assert sv.cost_routes(unreachable, np.array([[0, BLOCKED, 0]], np.uint8), [(0, 2)], 4)["status"].tolist() == [2]
    # status 4 on a hand-made field that is not a fixed point: the route stops and is kept
    cost, pen, kept = cost_cases.stuck_field()
    got = sv.cost_routes(cost, pen, [(0, 0)], 9)
    assert got["status"].tolist() == [4] and got["length"].tolist() == [3] and got["cells"][0, :3].tolist() == [list(c) for c in kept]
    assert sv.cost_routes(cost, pen, np.zeros((0, 2), np.int32), 3)["cells"].shape == (0, 3, 2)
    for bad in (dict(capacity=0), dict(capacity=65536), dict(starts=[(0, 0, 0)]), dict(starts=[(0.5, 0)]), dict(cost=cost.astype(np.int64)), dict(cost=cost[:2]),
                dict(pen=pen.astype(np.int8))):
        with pytest.raises(ValueError):
            sv.cost_routes(**dict(dict(cost=cost, pen=pen, starts=[(0, 0)], capacity=4), **bad))


def test_cells_of_world_points(sv):
    words = sv.occupancy_map_params((0, 8), (-2, 2), 2)  # top 16, left 4, 16 x 8 cells of 0.5 m
    xy = np.array([[7.9, 1.9], [0.0, -2.0], [7.5, 1.5], [8.0, 0.0], [0.0, 2.0], [-0.01, 0.0], [np.nan, 0.0], [1e300, 0.0]])
    assert sv.occupancy_cells_of(words, xy).tolist() == [[0, 0], [15, 7], [0, 0], [-1, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1]]
    inside, r, c = sv.clearance_cells(words, sv.occupancy_pose(xy[:3, 0], xy[:3, 1], 0.0), [(0.0, 0.0)])  # clearance_cells' rule
    assert inside.all() and np.stack([r[:, 0], c[:, 0]], -1).tolist() == sv.occupancy_cells_of(words, xy[:3]).tolist()
    assert sv.occupancy_cells_of(words, xy).dtype == np.int32 and sv.occupancy_cells_of(words, xy[0]).shape == (2,)


def _c_field_call(L, base, **kw):
    a = dict(base, **kw)
    return L.sv_cost_to_goal_device(a["pen"], a["rows"], a["cols"], a["goals"], a["n_goals"], a["init"], a["sweeps"], a["cost"], a["ws"], a["ws_bytes"], a["info"], a["stream"])


def _c_routes_call(L, base, **kw):
    a = dict(base, **kw)
    return L.sv_cost_routes_device(a["cost"], a["pen"], a["rows"], a["cols"], a["starts"], a["n_routes"], a["capacity"], a["cells"], a["length"], a["status"], a["stream"])


def _c_cells_call(L, base, **kw):
    a = dict(base, **kw)
    return L.sv_cost_cells_device(a["d2"], a["rows"], a["cols"], a["radius"], a["r2_block"], a["soft"], a["weight"], a["pen"], a["stream"])


def test_validation_needs_no_device(sv, eng):
    """Every refused argument raises ValueError in Python; the C entries return SV_ERR_ARG on host buffers, which stay untouched: the checks
    run before any HIP call."""
    pen = np.zeros((4, 6), np.uint8)
    for form in (sv.cost_to_goal, sv.cost_to_goal_relax):
        for bad in (dict(pen=pen.astype(np.int8)), dict(pen=pen[0]), dict(goals=np.zeros((0, 2), np.int32)), dict(goals=np.zeros((1025, 2), np.int32)),
                    dict(goals=[(0, 0, 0)]), dict(goals=[(0.5, 0.0)]), dict(pen=np.zeros((2001, 4000), np.uint8))):
            with pytest.raises(ValueError):
                form(**dict(dict(pen=pen, goals=[(0, 0)]), **bad))

    L = eng.cost_lib()
    need = ctypes.c_size_t(0)
    # the sweeps' 1024 words, the twin buffer, two sets of dirty bytes: each rounded up to 16
    assert L.sv_cost_to_goal_workspace(4, 6, ctypes.byref(need)) == 0 and need.value == 4096 + 96 + 2 * 16
    assert L.sv_cost_to_goal_workspace(2000, 2000, ctypes.byref(need)) == 0 and need.value == 4096 + 16000000 + 2 * 1024
    assert L.sv_cost_to_goal_workspace(2000, 4000, ctypes.byref(need)) == 0
    assert L.sv_cost_to_goal_workspace(1, 1, ctypes.byref(need)) == 0 and need.value == 4096 + 16 + 32
    for rows, cols, out in ((0, 1, need), (1, 0, need), (32769, 1, need), (1, 40000, need), (-1, 1, need), (2001, 4000, need), (32768, 32768, need), (4, 6, None)):
        assert L.sv_cost_to_goal_workspace(rows, cols, None if out is None else ctypes.byref(out)) == SV_ERR_ARG and need.value == 4096 + 16 + 32
        assert L.sv_last_error(None).startswith(b"sv_cost_to_goal_workspace")

    names = ("pen", "goals", "cost", "ws", "info", "d2", "starts", "cells", "length", "status")
    bufs = {k: np.full(8192, 0x5A, np.uint8) for k in names}
    ptr = lambda name: bufs[name].ctypes.data + (-bufs[name].ctypes.data) % 16  # noqa: E731
    ws_bytes = 4096 + 96 + 32
    base = dict(pen=ptr("pen"), rows=4, cols=6, goals=ptr("goals"), n_goals=2, init=1, sweeps=2, cost=ptr("cost"), ws=ptr("ws"), ws_bytes=ws_bytes, info=ptr("info"),
                stream=None)
    cases = [dict(sweeps=3), dict(sweeps=0), dict(sweeps=1), dict(sweeps=-2), dict(sweeps=1026), dict(sweeps=1025), dict(rows=2001, cols=4000), dict(rows=0), dict(cols=0),
             dict(rows=32769), dict(cols=-1), dict(n_goals=0), dict(n_goals=1025), dict(n_goals=-1), dict(init=2), dict(init=-1), dict(pen=None), dict(goals=None),
             dict(cost=None), dict(ws=None), dict(info=None), dict(goals=ptr("goals") + 2), dict(cost=ptr("cost") + 1), dict(info=ptr("info") + 2), dict(ws=ptr("ws") + 8),
             dict(ws_bytes=ws_bytes - 1), dict(ws_bytes=0), dict(cost=ptr("pen")), dict(cost=ptr("pen") + 20), dict(cost=ptr("goals") + 12), dict(cost=ptr("ws") + 4096),
             dict(cost=ptr("info") - 92), dict(info=ptr("ws") + 16), dict(info=ptr("pen") + 20), dict(info=ptr("goals")), dict(ws=ptr("pen") - 4208),
             dict(ws=ptr("goals") - 4096)]
    for kw in cases:
        rc, text = _c_field_call(L, base, **kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_cost_to_goal:"), (sorted(kw), rc, text)

    cbase = dict(d2=ptr("d2"), rows=4, cols=6, radius=3, r2_block=9, soft=2, weight=5, pen=ptr("pen"), stream=None)
    for kw in (dict(r2_block=10), dict(r2_block=-1), dict(radius=0), dict(radius=255), dict(soft=-1), dict(soft=255), dict(weight=-1), dict(weight=255), dict(rows=0),
               dict(cols=32769), dict(d2=None), dict(pen=None), dict(d2=ptr("d2") + 1), dict(pen=ptr("d2")), dict(pen=ptr("d2") + 47)):
        rc, text = _c_cells_call(L, cbase, **kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_cost_cells:"), (sorted(kw), rc, text)

    rbase = dict(cost=ptr("cost"), pen=ptr("pen"), rows=4, cols=6, starts=ptr("starts"), n_routes=3, capacity=5, cells=ptr("cells"), length=ptr("length"),
                 status=ptr("status"), stream=None)
    for kw in (dict(n_routes=-1), dict(n_routes=65536), dict(capacity=0), dict(capacity=65536), dict(rows=0), dict(rows=2001, cols=4000), dict(cost=None), dict(pen=None),
               dict(starts=None), dict(cells=None), dict(length=None), dict(status=None), dict(cost=ptr("cost") + 2), dict(starts=ptr("starts") + 1), dict(cells=ptr("cells") + 2),
               dict(length=ptr("length") + 1), dict(status=ptr("status") + 2), dict(cells=ptr("cost") + 92), dict(cells=ptr("pen") + 20), dict(length=ptr("starts") + 20),
               dict(status=ptr("cells") + 56), dict(status=ptr("length") + 8), dict(length=ptr("cells"))):
        rc, text = _c_routes_call(L, rbase, **kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_cost_routes:"), (sorted(kw), rc, text)
    # legal and without work: no route - nothing is enqueued, with or without buffers
    assert _c_routes_call(L, rbase, n_routes=0) == 0 and _c_routes_call(L, rbase, n_routes=0, starts=None, cells=None, length=None, status=None) == 0
    assert all((b == 0x5A).all() for b in bufs.values())
    assert eng.debug_cost_to_goal(0, None) == 0
    for bad in (-1, 2, 17):
        assert eng.debug_cost_to_goal(bad, None) == SV_ERR_ARG and L.sv_last_error(None).startswith(b"sv_debug_cost_to_goal")
    assert eng.debug_cost_to_goal(0, None) == 0


def test_header_build_and_loader_agree(eng):
    """The library exports the five entries the header declares for group (N), and build.py lists the new sources and header."""
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(sv_[a-z_]*cost[a-z_]*)\s*\(", src))
    assert declared == {"sv_cost_cells_device", "sv_cost_to_goal_workspace", "sv_cost_to_goal_device", "sv_cost_routes_device", "sv_debug_cost_to_goal"}
    L = eng.cost_lib()
    assert all(hasattr(L, n) for n in declared)
    assert len(L.sv_cost_to_goal_device.argtypes) == 12 and len(L.sv_cost_routes_device.argtypes) == 11 and len(L.sv_cost_cells_device.argtypes) == 9
    assert text.index("/* ---- (M)") < text.index("/* ---- (N)") < text.index("/* ---- (A)")
    build = util.pkg("build")
    assert "cost_kernels.hip" in build.SOURCES and "cost.cpp" in build.SOURCES and "cost_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("cost_kernels.hip", "cost.cpp", "cost_kernels.h"))
    sv_mod = util.pkg("stereo_vision.sv")
    assert all(n in sv_mod.__doc__ for n in ("cost_cells", "cost_to_goal", "cost_to_goal_relax", "cost_routes", "occupancy_cells_of"))


GOAL_XY, START_XY = [(12.0, 3.0), (100.0, 0.0)], [(3.25, -1.5), (20.0, -15.0), (-50.0, 0.0), (5.0, 1.0)]  # one goal and one start lie outside the map


def _map_results(world):
    world.clearance(1.0)
    field = world.cost_to_goal(GOAL_XY, 0.5, soft_m=1.0, weight=5)
    routes, xy = world.routes(START_XY, capacity=400)
    return field, routes, xy


def test_map_class_on_cpu_tensors(sv):
    """rig.OccupancyMap.cost_to_goal / routes on CPU tensors run the numpy definitions: the host logic without a GPU."""
    import torch
    (world,) = _fused_recovery_maps(sv, ["cpu"])
    with pytest.raises(ValueError):
        world.cost_to_goal(GOAL_XY, 0.5)  # no clearance field yet
    world.clearance(1.0)
    with pytest.raises(ValueError):
        world.routes(START_XY)  # no cost-to-goal field yet
    for bad in (dict(block_m=1.01), dict(block_m=-1.0), dict(block_m=float("nan")), dict(soft_m=-0.5)):  # 1.01 m are 5 cells > R = 4
        with pytest.raises(ValueError):
            world.cost_to_goal(**dict(dict(goal_xy=GOAL_XY, block_m=0.5), **bad))
    field, routes, xy = _map_results(world)
    d2 = sv.occupancy_clearance(world.logodds.numpy(), 4, 85)
    pen = sv.cost_cells(d2, 4, soft=4, weight=5, radius=4)  # 0.5 m are 2 cells, 1 m are 4
    goals = sv.occupancy_cells_of(world.words, GOAL_XY)
    assert goals.tolist() == [[71, 67], [-1, -1]] and (pen == BLOCKED).sum() > (d2 == 0).sum() > 50 and ((pen > 0) & (pen < BLOCKED)).any()
    want = sv.cost_to_goal(pen, goals)
    assert field.converged and field.cost.dtype == torch.int32 and _bits(field.cost.numpy(), want) and want[71, 67] == 0
    ref = sv.cost_routes(want, pen, sv.occupancy_cells_of(world.words, START_XY), 400)
    assert all(_bits(getattr(routes, k).numpy(), ref[k]) for k in ROUTE_KEYS)
    assert ref["status"].tolist() == [0, 0, 1, 0] and ref["length"][0] > 30
    Xw, Yw = world.centres()
    n = int(ref["length"][0])
    assert xy.shape == (4, 400, 2) and xy.dtype == np.float64 and np.isnan(xy[0, n:]).all() and np.isnan(xy[2]).all()
    assert np.array_equal(xy[0, :n, 0], Xw[ref["cells"][0, :n, 0]]) and np.array_equal(xy[0, :n, 1], Yw[ref["cells"][0, :n, 1]])
    assert abs(xy[0, 0, 0] - 3.25) <= 0.125 and abs(xy[0, n - 1, 0] - 12.0) <= 0.125  # from the start's cell to the goal's
    one, one_xy = world.routes(START_XY[0], capacity=5)
    assert one.status.tolist() == [3] and one.length.tolist() == [5] and one_xy.shape == (1, 5, 2)


# ---------------------------------------------------------------------------------------------------------------- GPU

def _field_gpu(eng, pen, goals, **kw):
    res = eng.occupancy_cost_to_goal(_cuda(pen), goals, **kw)
    return res, res.cost.cpu().numpy()


class _Raw:
    """The C entry on buffers of its own: a field that can be started, continued and read back sweep count by sweep count."""

    def __init__(self, eng, pen, goals):
        import torch
        self.L, self.pen, self.goals = eng.cost_lib(), _cuda(pen), _cuda(np.asarray(goals, np.int32))
        self.rows, self.cols = pen.shape
        need = ctypes.c_size_t(0)
        assert self.L.sv_cost_to_goal_workspace(self.rows, self.cols, ctypes.byref(need)) == 0
        self.cost = torch.full(pen.shape, -7, dtype=torch.int32, device="cuda")  # nothing is assumed of what the buffers held
        self.ws = torch.full((need.value,), 0xA5, dtype=torch.uint8, device="cuda")
        self.info = torch.full((4,), -7, dtype=torch.int32, device="cuda")

    def run(self, init, sweeps):
        import torch
        rc = self.L.sv_cost_to_goal_device(self.pen.data_ptr(), self.rows, self.cols, self.goals.data_ptr(), self.goals.shape[0], init, sweeps, self.cost.data_ptr(),
                                           self.ws.data_ptr(), self.ws.numel(), self.info.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, self.L.sv_last_error(None)
        return self.cost.cpu().numpy(), self.info.cpu().numpy().tolist()


FIELD_NAMES = sorted(cost_cases.field_cases())


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIELD_NAMES)
def test_field_equals_the_definition(sv, eng, fields, name):
    """The smallest shapes at which the sweep kernel can go wrong - see cost_cases.field_cases - against Dijkstra, through the engine; the
    cap is derived, not measured: a sweep that relaxes every dirty tile at least once finalises at least one more cell of every shortest
    path, so rows x cols sweeps always suffice."""
    pen, goals, want = fields[name]
    res, got = _field_gpu(eng, pen, goals, max_sweeps=pen.size + (pen.size & 1))
    print(name, "sweeps", res.sweeps)
    assert res.converged and _bits(got, want)
    if name in ("all blocked", "no valid goal"):
        assert (got == INF).all() and res.sweeps == 1  # converged after the first round: its first sweep confirms
    if name == "pen 254":
        assert got.max() == 64 * (254 + 14)


@pytest.mark.gpu
def test_serpentine_and_the_c_entry(sv, eng, fields):
    """The serpentine - tiles go clean and dirty again - through the C entry and the engine; the resumed call, the unconverged call twice,
    and the variant that runs every tile."""
    import torch
    pen, goals, want = fields["serpentine"]
    assert (want != INF).sum() > 8400 and want.max() > 85000
    res, got = _field_gpu(eng, pen, goals, max_sweeps=pen.size)
    print("serpentine: sweeps", res.sweeps)
    assert res.converged and _bits(got, want) and res.sweeps > 4

    # resume: 8 + 8 sweeps equal 16, in cost and in the summed info[1]
    a, b = _Raw(eng, pen, goals), _Raw(eng, pen, goals)
    first, info1 = a.run(1, 8)
    second, info2 = a.run(0, 8)
    whole, info = b.run(1, 16)
    assert _bits(second, whole) and info1[1] + info2[1] == info[1] == 16 and info[0] == info2[0] == 1 and info[2:] == info1[2:] == [0, 0]
    assert not np.array_equal(first, second) and (second <= first).all()
    # unconverged it is an upper bound of the definition, and the same bits and info every time
    assert (whole >= want).all() and (whole > want).any()
    again, info_again = _Raw(eng, pen, goals).run(1, 8)
    assert _bits(again, first) and info_again == info1
    # continued to the end through the same entry
    for _ in range(pen.size // 64):
        last, info = a.run(0, 64)
        if info[0] == 0:
            break
    assert info[0] == 0 and _bits(last, want)

    # variant 1 runs every tile in every sweep: the same field, the same sweeps, more tiles
    tiles = 3 * 3
    counted = {}
    try:
        for variant in (0, 1):
            counters = torch.zeros(2, dtype=torch.int64, device="cuda")
            assert eng.debug_cost_to_goal(variant, counters) == 0
            r, g = _field_gpu(eng, pen, goals, max_sweeps=pen.size)
            torch.cuda.synchronize()
            counted[variant] = (r.sweeps, r.converged, g, counters.cpu().numpy().tolist())
    finally:
        assert eng.debug_cost_to_goal(0, None) == 0
    print("serpentine: tiles run, inner iterations", counted[0][3], counted[1][3], "of", tiles, "tiles x", res.sweeps, "sweeps")
    assert counted[0][:2] == counted[1][:2] == (res.sweeps, True) and _bits(counted[0][2], want) and _bits(counted[1][2], want)
    launched = 16 * ((res.sweeps + 15) // 16)  # rounds of 16 sweeps; the confirming sweep is the last that counts
    assert counted[1][3][0] == tiles * launched and 0 < counted[0][3][0] < tiles * res.sweeps
    assert counted[0][3][1] >= counted[0][3][0]


@pytest.mark.gpu
def test_field_buffers_and_refusals(sv, eng, fields):
    import torch
    pen, goals, want = fields["65x65 three goals"]
    t_pen = _cuda(pen)
    out = torch.empty(pen.shape, dtype=torch.int32, device="cuda")
    res = eng.occupancy_cost_to_goal(t_pen, _cuda(goals), out=out, round=2)
    assert res.cost is out and _bits(out.cpu().numpy(), want)
    again = eng.occupancy_cost_to_goal(t_pen, goals.tolist(), out=out, workspace=res.workspace, round=1024)
    assert again.workspace is res.workspace and again.sweeps == res.sweeps and _bits(out.cpu().numpy(), want)
    s_pen, s_goals, s_want = fields["serpentine"]
    short = eng.occupancy_cost_to_goal(_cuda(s_pen), s_goals, max_sweeps=1)  # made even: two sweeps
    assert not short.converged and short.sweeps == 2 and (short.cost.cpu().numpy() >= s_want).all()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        on_side = eng.occupancy_cost_to_goal(t_pen, goals)
    side.synchronize()
    assert _bits(on_side.cost.cpu().numpy(), want)
    for bad in (dict(pen=t_pen.cpu()), dict(pen=t_pen.view(torch.int8)), dict(pen=t_pen[:, :60]), dict(goals=np.zeros((0, 2), np.int32)), dict(goals=_cuda(goals).long()),
                dict(round=3), dict(round=0), dict(round=1026), dict(max_sweeps=0), dict(out=out[:60]), dict(out=out.float()), dict(workspace=res.workspace[:100]),
                dict(pen=torch.zeros((2001, 4000), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            eng.occupancy_cost_to_goal(**dict(dict(pen=t_pen, goals=goals), **bad))


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1, 15, 16, 17])
def test_cost_cells_equal_the_definition(sv, eng, cols):
    """Values at r2_block - 1, r2_block, r2_block + 1, 65535 and both sides of every root k^2, at the widths around a 16-byte access -
    and from a tensor that starts 2 bytes past a 16-byte boundary, which takes the cell-by-cell path."""
    import torch
    R, r2_block = 40, 1444
    special = [r2_block - 1, r2_block, r2_block + 1, 65535, 0, 1, 2] + [k * k - 1 for k in range(1, 256)] + [k * k for k in range(1, 256)]
    rows = -(-len(special) * 2 // cols)
    d2 = np.resize(np.array(special, np.uint16), (rows, cols))
    for soft, weight in ((0, 0), (40, 7), (254, 254), (39, 1)):
        want = sv.cost_cells(d2, r2_block, soft, weight, radius=R)
        got = eng.cost_cells(_cuda(d2), R, r2_block, soft, weight)
        assert _bits(got.cpu().numpy(), want) and (want == BLOCKED).any()
        raw = torch.zeros(2 * d2.size + 2, dtype=torch.uint8, device="cuda")
        raw[2:].copy_(_cuda(d2.view(np.uint8).reshape(-1)))
        shifted = raw[2:].view(torch.uint16).view(rows, cols)
        out = torch.zeros(d2.size + 3, dtype=torch.uint8, device="cuda")[3:].view(rows, cols)
        assert shifted.data_ptr() % 16 == 2 and eng.cost_cells(shifted, R, r2_block, soft, weight, out=out) is out and _bits(out.cpu().numpy(), want)
    for bad in (dict(r2_block=R * R + 1), dict(r2_block=-1), dict(soft=255), dict(weight=255), dict(radius=0), dict(radius=255), dict(d2=_cuda(d2).cpu()),
                dict(d2=_cuda(d2.astype(np.int16))), dict(out=torch.zeros((rows, cols + 1), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(ValueError):
            eng.cost_cells(**dict(dict(d2=_cuda(d2), radius=R, r2_block=r2_block), **bad))


def _routes_gpu(eng, cost, pen, starts, capacity):
    res = eng.cost_routes(_cuda(np.array(cost)), _cuda(pen), starts, capacity)  # a copy: the references are read-only
    return {k: getattr(res, k).cpu().numpy() for k in ROUTE_KEYS}


@pytest.mark.gpu
def test_routes_equal_the_definition(sv, eng, fields):
    """Groups of 8 lanes that are partly filled and a second wavefront (K = 0 .. 65); starts that reach the goal at different lengths
    within one wavefront, so that finished groups idle beside running ones; every status."""
    rng = np.random.default_rng(11)
    pen, goals, want = fields["serpentine"]
    n = pen.shape[0]
    for K in (0, 1, 7, 8, 9, 65):
        # along the serpentine: from one cell off the goal to its far end, and a few walls and cells outside the map between them
        starts = np.stack([rng.integers(-1, n + 1, K), rng.integers(-1, n + 1, K)], -1).astype(np.int32)
        if K:
            starts[0] = (0, 1)
            starts[-1] = (n - 2, 0)
        ref = sv.cost_routes(want, pen, starts, 9000)
        got = _routes_gpu(eng, want, pen, starts, 9000)
        assert all(_bits(got[k], ref[k]) for k in ROUTE_KEYS), K
        if K >= 7:
            assert ref["length"].max() > 8000 and len(set(ref["length"].tolist())) >= 4 and {0, 2}.issubset(set(ref["status"].tolist()))
    for name in ("hand", "130x130 three goals", "corner 64,64"):
        pen, goals, want = fields[name]
        rows, cols = pen.shape
        starts = np.stack(np.mgrid[-1:rows + 1, -1:cols + 1], -1).reshape(-1, 2)[:: max(1, (rows + 2) * (cols + 2) // 300)].astype(np.int32)
        for capacity in (1, 7, 300):
            ref = sv.cost_routes(want, pen, starts, capacity)
            got = _routes_gpu(eng, want, pen, starts, capacity)
            assert all(_bits(got[k], ref[k]) for k in ROUTE_KEYS), (name, capacity)
    # a route exactly capacity long reaches its goal; one cell less and it does not
    exact = _routes_gpu(eng, HAND_COST, HAND_PEN, np.array([[2, 6]], np.int32), 7)
    assert exact["status"].tolist() == [0] and exact["length"].tolist() == [7] and exact["cells"][0].tolist() == [list(c) for c in HAND_ROUTE]
    assert _routes_gpu(eng, HAND_COST, HAND_PEN, np.array([[2, 6]], np.int32), 6)["status"].tolist() == [3]
    cost, spen, kept = cost_cases.stuck_field()
    stuck = _routes_gpu(eng, cost, spen, np.array([[0, 0], [0, 4], [0, 2]], np.int32), 9)
    assert stuck["status"].tolist() == [4, 0, 4] and stuck["length"].tolist() == [3, 1, 1] and stuck["cells"][0, :3].tolist() == [list(c) for c in kept]
    assert all(_bits(stuck[k], sv.cost_routes(cost, spen, [(0, 0), (0, 4), (0, 2)], 9)[k]) for k in ROUTE_KEYS)
    import torch
    t_cost, t_pen = _cuda(cost), _cuda(spen)
    for bad in (dict(cost=t_cost.cpu()), dict(cost=t_cost.float()), dict(pen=t_pen[:2]), dict(pen=t_pen.view(torch.int8)), dict(capacity=0), dict(capacity=65536),
                dict(starts=np.zeros((2, 3), np.int32)), dict(starts=torch.zeros((2, 2), dtype=torch.int64, device="cuda"))):
        with pytest.raises(ValueError):
            eng.cost_routes(**dict(dict(cost=t_cost, pen=t_pen, starts=[(0, 0)], capacity=4), **bad))


@pytest.mark.gpu
def test_map_class_on_the_device(sv, eng):
    """rig.OccupancyMap on the device against the class on CPU tensors: the recovery scene's field and routes, and again after another
    frame into the same buffers."""
    world, cpu = _fused_recovery_maps(sv, ["cuda", "cpu"])
    (field, routes, xy), (field_cpu, routes_cpu, xy_cpu) = _map_results(world), _map_results(cpu)
    assert field.cost.is_cuda and field.converged and field.sweeps >= 2 and _bits(field.cost.cpu().numpy(), field_cpu.cost.numpy())
    assert all(_bits(getattr(routes, k).cpu().numpy(), getattr(routes_cpu, k).numpy()) for k in ROUTE_KEYS) and np.array_equal(xy, xy_cpu, equal_nan=True)
    assert routes_cpu.status.tolist() == [0, 0, 1, 0]
    stripes = np.ones((49, 49), np.uint8)
    stripes[:, ::7] = 2
    for m in (world, cpu):
        m.update(stripes[None], sv.occupancy_pose(9.0, 4.0, -0.8)[None], RECOVERY_FRAME)
    (again, routes, xy), (again_cpu, routes_cpu, xy_cpu) = _map_results(world), _map_results(cpu)
    assert again.cost is field.cost and _bits(again.cost.cpu().numpy(), again_cpu.cost.numpy())
    assert all(_bits(getattr(routes, k).cpu().numpy(), getattr(routes_cpu, k).numpy()) for k in ROUTE_KEYS) and np.array_equal(xy, xy_cpu, equal_nan=True)


@pytest.mark.gpu
def test_cli_writes_the_route(sv, eng, drive, tmp_path, capsys):
    from PIL import Image
    _, states, _, _, _ = drive
    n = 2
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    ls, rs = _drive_frames(n)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    xyyaw = np.array([[0.0, 0.0, 0.0], [0.9, 0.1, 0.02]])
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("".join("%r %r %r\n" % tuple(float(v) for v in row) for row in xyyaw))
    out = str(tmp_path / "map.png")
    common = ["-k", str(tmp_path / "kitti"), "--batch", "2"]
    with_map = ["--occupancy-map", out, "--poses", str(tmp_path / "poses.txt")]
    for bad in (["--goal", "30,5"], with_map + ["--goal", "30,5"], ["--occupancy-map", out, "--clearance", "2.0", "--goal", "30,5"], with_map + ["--clearance", "2.0", "--goal", "30"],
                with_map + ["--clearance", "2.0", "--goal", "30,x"], with_map + ["--clearance", "2.0", "--goal", "30,5,1"], with_map + ["--clearance", "2.0", "--goal", "nan,5"]):
        with pytest.raises(SystemExit):
            sv.main(common + bad)
    assert not os.path.exists(out)
    # the definition on CPU tensors: the map of the two frames, its field with 2 m blocked, the route from the last pose
    ranges = sv.occupancy_map_cover(xyyaw, sv.CLI_TOP_VIEW["x_range"], sv.CLI_TOP_VIEW["y_range"])
    cpu = util.pkg("rig").OccupancyMap(ranges[0], ranges[1], 10, device="cpu")
    cpu.update(states[:2], sv.occupancy_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2]), CLI_GRID)
    d2 = cpu.clearance(2.0).numpy()
    pen = sv.cost_cells(d2, 400, radius=20)
    goal_xy = next(g for g in ((30.0, 5.0), (30.0, -5.0), (20.0, 0.0), (-20.0, 10.0)) if pen[tuple(sv.occupancy_cells_of(cpu.words, g))] != BLOCKED)
    field = cpu.cost_to_goal(goal_xy, 2.0)
    routes, xy = cpu.routes(xyyaw[-1, :2])
    length, status = int(routes.length[0]), int(routes.status[0])
    assert status == 0 and length > 100 and (pen == BLOCKED).any()
    capsys.readouterr()
    sv.main(common + with_map + ["--clearance", "2.0", "--goal", "%r,%r" % goal_xy])
    printed = capsys.readouterr().out
    start = routes.cells[0, 0].tolist()
    assert "route: status 0, %d cells, cost at the start %d\n" % (length, int(field.cost[start[0], start[1]])) in printed
    with open(tmp_path / "route.txt") as f:
        lines = [line.split() for line in f]
    assert len(lines) == length
    assert [[int(r), int(c)] for r, c, _, _ in lines] == routes.cells[0, :length].tolist()
    assert np.array_equal(np.array([[float(x), float(y)] for _, _, x, y in lines]), xy[0, :length])
