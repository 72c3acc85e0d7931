"""The voxel map flattened into an occupancy map (group (V)): stereo_vision.sv.voxel_map_flatten against its plain-loop form and hand
numbers, and engine.voxel_map_flatten / rig.VoxelMap.flatten / rig.OccupancyMap.load_voxels against the definition.  Every comparison is
shape, dtype and bytes."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
import voxel_flatten_cases as flatten
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_map_cases import BOX16, cell_points, one_frame

SV_ERR_ARG = -1
FIELDS = ("logodds", "last_seen", "floor", "top", "cells", "stats")
DRAWN, OUTSIDE, BELOW, GROUND, OBSTACLE, OVERHEAD, OCCUPIED, FREE = range(8)


def _differ(got, want, fields=FIELDS):
    return [k for k in fields if not (got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes())]


def _define(sv, case):
    state, seq = sv.voxel_map_state(sv.voxel_map_params(**case["params"])), 0
    for call in case["calls"]:
        sv.voxel_map_insert(state, *call, seq0=seq)
        seq += call[0].shape[0]
    return state


@pytest.fixture(scope="module")
def all_cases():
    return flatten.all_cases()


@pytest.fixture(scope="module")
def defined(sv, all_cases):
    """Per case the numpy form's result, computed once and left as it is."""
    return {name: sv.voxel_map_flatten(_define(sv, c), c["flat"], c["spec"], **c["kw"]) for name, c in all_cases.items()}


def _cell(flat, x, y):
    """(row, col) of the flat cell that holds the world point (x, y)."""
    return flat["top"] - 1 - int(np.floor(x * flat["scale"])), flat["left"] - 1 - int(np.floor(y * flat["scale"]))


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_vectorised_against_brute(sv, all_cases, defined):
    for name, c in all_cases.items():
        brute = sv.voxel_map_flatten_brute(_define(sv, c), c["flat"], c["spec"], **c["kw"])
        assert _differ(defined[name], brute) == [], (name, defined[name]["stats"].tolist(), brute["stats"].tolist())


def test_hand_numbers(sv, all_cases, defined):
    """The threshold case by hand: zq 949 is below, 950 .. 1049 ground, 1050 .. 1399 obstacle, 1400 and 1401 overhead over a floor at 1000."""
    c, d = all_cases["threshold"], defined["threshold"]
    assert d["stats"].tolist() == [9, 0, 1, 3, 3, 2, 3, 3]
    kinds = []
    for k, zq in enumerate(flatten.THRESHOLD_ZQ):
        r, col = _cell(c["flat"], 1.5 + k, 2.5)
        kinds.append((d["cells"][r, col].tolist(), int(d["logodds"][r, col]), int(d["last_seen"][r, col]), int(d["top"][r, col]), int(d["floor"][r, col])))
    below, ground, obstacle, overhead = ([0, 0, 0], 0, -1, -1), ([1, 0, 0], -40, 0), ([0, 1, 0], 85, 0), ([0, 0, 1], 0, -1, -1)
    want = [below + (1000,)] + [ground + (zq, 1000) for zq in (950, 951, 1049)] + [obstacle + (zq, 1000) for zq in (1050, 1051, 1399)] + [overhead + (1000,)] * 2
    assert kinds == want
    assert (d["floor"] == 1000).all()  # mode 0: the floor of every cell


def test_the_cases_show_what_they_are_for(sv, all_cases, defined):
    d = defined
    for name, (xr, yr) in flatten.SHAPES.items():
        got = d["shape_" + name]
        assert got["logodds"].shape == (xr[1] - xr[0], yr[1] - yr[0]) and got["stats"][DRAWN] > 0 and got["stats"][OUTSIDE] > 0, name
        if name != "1x1":
            assert (got["stats"][[GROUND, OBSTACLE, OVERHEAD, OCCUPIED, FREE]] > 0).all() and (got["last_seen"] == -1).any(), name
    assert all_cases["shape_negative"]["flat"]["top"] < 0 and all_cases["shape_negative"]["flat"]["left"] < 0
    assert d["shape_65x70_absolute"]["stats"][BELOW] == 0 and (d["shape_65x70_radius8"]["floor"] >= 0).all()
    for name in ("incommensurate_size03_scale2", "incommensurate_size05_scale4"):
        assert (d[name]["stats"][[DRAWN, OUTSIDE, GROUND, OBSTACLE, OVERHEAD]] > 50).all(), name
    # the border case: three voxels per axis, the first with its centre on a flat cell's border exactly
    c = all_cases["border"]
    state = _define(sv, c)
    rows = sv.voxel_map_rows(state, dtype="f64")
    on_x, on_y = rows["xyz"][:, 0] * 2.0, rows["xyz"][:, 1] * 2.0
    assert sorted(set(state["S"][:, 0].tolist())) == [65534, 65535, 65536] and (state["n"] == 2).all()
    assert (on_x == np.floor(on_x)).sum() == 1 and (on_y == np.floor(on_y)).sum() == 1
    assert np.abs(on_x - np.round(on_x)).min() == 0 and sorted(np.abs(on_x - np.round(on_x)))[1:3] == [2.0 ** -16, 2.0 ** -16]
    flat = c["flat"]
    for k in range(3):  # X = 2.5 + 2 k (-+ 1 / 131072): the cells of gx = 5 + 4 k, 4 + 4 k and 5 + 4 k
        gx = [5, 4, 5][k] + 4 * k
        assert d["border"]["cells"][flat["top"] - 1 - gx, flat["left"] - 1 - 7, 0] == 1, k
        assert d["border"]["cells"][flat["top"] - 1 - 7, flat["left"] - 1 - gx, 0] == 1, k
    # the contention case: 70 voxels in one flat cell, one in each neighbour
    got = d["contention"]
    r, col = _cell(all_cases["contention"]["flat"], 5.5, 5.5)
    assert got["cells"][r, col].tolist() == [1, 7, 62] and got["cells"][r, col].sum() >= 64
    assert all(got["cells"][r + dr, col + dc].sum() == 1 for dr in (-1, 0, 1) for dc in (-1, 0, 1) if (dr, dc) != (0, 0))
    assert got["top"][r, col] == 7 * 256 + 128 and got["floor"][r, col] == 128 and got["logodds"][r, col] == 350
    four, wholly = d["outside_four_sides"], d["outside_wholly"]
    pts = all_cases["outside_four_sides"]["calls"][0][0][0]
    assert (pts[:, 0] < 5).any() and (pts[:, 0] > 9).any() and (pts[:, 1] < 6).any() and (pts[:, 1] > 11).any()
    assert four["stats"][DRAWN] > 20 and four["stats"][OUTSIDE] > 100
    assert wholly["stats"].tolist() == [0, int(four["stats"][:2].sum()), 0, 0, 0, 0, 0, 0] and not wholly["logodds"].any() and (wholly["floor"] == -1).all()
    # the ring: A's floor reaches 8 cells and no further, and makes B an obstacle from radius 8 on; the wall's column stands on G's floor from radius 1 on
    ax, ay = flatten.RING_AT
    flat = all_cases["ring_radius8"]["flat"]
    at = lambda x, y: _cell(flat, x + 0.5, y + 0.5)  # noqa: E731
    r8, r1, r0 = d["ring_radius8"], d["ring_radius1"], d["ring_radius0"]
    assert r8["floor"][at(ax + 8, ay)] == 10 and r8["floor"][at(ax - 8, ay - 8)] == 10 and r8["floor"][at(ax - 9, ay)] == -1 and r8["floor"][at(ax, ay - 9)] == -1
    assert r1["floor"][at(ax + 1, ay + 1)] == 10 and r1["floor"][at(ax + 2, ay)] == -1 and r0["floor"][at(ax + 1, ay)] == -1
    assert r8["cells"][at(ax + 8, ay + 8)].tolist() == [0, 1, 0] and r1["cells"][at(ax + 8, ay + 8)].tolist() == [1, 0, 0]
    assert r8["cells"][at(ax + 9, ay)].tolist() == [1, 0, 0] and r8["floor"][at(ax + 9, ay)] == 384  # from B, 8 cells away: A is 9 away
    assert r0["cells"][at(41, 40)].tolist() == [1, 2, 0] and r1["cells"][at(41, 40)].tolist() == [0, 3, 0] and r1["floor"][at(41, 40)] == 20
    for x, y in ((1, 1), (1, 62), (62, 1), (62, 62), (1, 30), (62, 30), (30, 1), (30, 62)):  # beside a corner or an edge: the window is clipped
        assert r0["cells"][at(x, y)].tolist() == [1, 0, 0] and r1["cells"][at(x, y)].tolist() == [0, 1, 0]
    assert r8["floor"][at(0, 0)] == 300 and r8["floor"][at(8, 8)] == 300 and r8["floor"][at(9, 9)] == 700 and r8["floor"][at(12, 12)] == 10  # the corner's voxel, its neighbour's, then A's
    small = d["ring_small_map"]
    assert small["logodds"].shape == (5, 3) and (small["floor"] == 20).all() and small["stats"][:2].tolist() == [4, 19]
    # the counts against min_obstacle and min_ground
    r, col = _cell(all_cases["counted_o2_g1"]["flat"], 4.5, 4.5)
    for mo in (2, 3, 4):
        for mg in (1, 2, 3):
            got = d["counted_o%d_g%d" % (mo, mg)]
            assert got["cells"][r, col].tolist() == [flatten.COUNTED["ground"], flatten.COUNTED["obstacle"], 0]
            want = 3 * 85 if mo <= 3 else (-2 * 40 if mg <= 2 else 0)
            assert got["logodds"][r, col] == want and got["last_seen"][r, col] == (0 if want else -1) and got["top"][r, col] == 1200
    # the clamps
    column, ground = _cell(all_cases["clamp_wide"]["flat"], 5.5, 5.5), _cell(all_cases["clamp_wide"]["flat"], 9.5, 9.5)
    assert d["clamp_default"]["cells"][column].tolist() == list(flatten.CLAMPED["column"]) and d["clamp_default"]["cells"][ground].tolist() == [flatten.CLAMPED["ground"], 0, 0]
    assert 34 * 85 > 350 and d["clamp_default"]["logodds"][column] == 350 and 6 * 40 > 200 and d["clamp_default"]["logodds"][ground] == -200
    assert 34 * 32767 > 2 ** 16 and d["clamp_wide"]["logodds"][column] == 32767 and d["clamp_wide"]["logodds"][ground] == -32767
    assert d["clamp_not_reached"]["logodds"][column] == 34 * 900 and d["clamp_not_reached"]["logodds"][ground] == -6 * 5000
    # the filters: each drops another voxel of the one cell
    r, col = _cell(all_cases["filter_none"]["flat"], 4.5, 4.5)
    seen = {k: (d["filter_" + k]["cells"][r, col].tolist(), int(d["filter_" + k]["floor"][r, col]), int(d["filter_" + k]["top"][r, col]), int(d["filter_" + k]["last_seen"][r, col]))
            for k in ("none", "min_n", "min_rows", "since")}
    assert seen == {"none": ([2, 1, 1], 128, 640, 1), "min_n": ([2, 1, 0], 384, 896, 1), "min_rows": ([1, 1, 1], 128, 640, 1), "since": ([2, 0, 1], 128, 384, 1)}
    for name in ("overflowed_local", "overflowed_absolute"):
        got = d[name]
        assert got["stats"].tolist() == [-1, 0, 0, 0, 0, 0, 0, 0] and not got["logodds"].any() and (got["last_seen"] == -1).all() and (got["top"] == -1).all()
        assert not got["cells"].any() and (got["floor"] == (-1 if name == "overflowed_local" else -77)).all()
    assert not d["empty"]["stats"].any() and (d["empty"]["floor"] == -1).all()


def test_params_and_refusals(sv):
    p = sv.voxel_map_params(**flatten.WIDE)
    assert sv.voxel_flatten_params(p) == dict(mode=1, z_ref_q=0, step_q=102, height_q=1024, radius=2, min_obstacle=1, min_ground=1)
    assert sv.voxel_flatten_params(p, z_ref=0.0, step=0.25, height=1.5, radius=0, min_obstacle=2, min_ground=3) == dict(
        mode=0, z_ref_q=512, step_q=128, height_q=768, radius=0, min_obstacle=2, min_ground=3)
    assert sv.voxel_flatten_params(p, z_ref=-1.001)["z_ref_q"] == -1 and sv.voxel_flatten_params(p, z_ref=-3.0)["z_ref_q"] == -1024  # floor(), below lo_z too
    for kw in (dict(step=2.0, height=2.0), dict(step=3.0), dict(step=0.0), dict(radius=-1), dict(radius=9), dict(radius=1.5), dict(z_ref=np.nan), dict(z_ref=np.inf),
               dict(step=np.nan), dict(height=np.inf), dict(min_obstacle=0), dict(min_ground=0), dict(height=1e9), dict(z_ref=1e9)):
        with pytest.raises(ValueError):
            sv.voxel_flatten_params(p, **kw)
    good = sv.voxel_flatten_params(p)
    assert sv.voxel_flatten_words(dict(good, reserved=[0] * 9)) == good
    for bad in (dict(good, reserved=[0, 0, 1]), dict(good, mode=2), dict(good, z_ref_q=2 ** 30), dict(good, height_q=2 ** 28), dict(good, step_q=0), {k: v for k, v in good.items() if k != "radius"}):
        with pytest.raises(ValueError):
            sv.voxel_flatten_words(bad)
    state = sv.voxel_map_state(p)
    flat = flatten.flat_words((0, 4), (0, 4), 1)
    for form in (sv.voxel_map_flatten, sv.voxel_map_flatten_brute):
        for kw in (dict(min_n=0), dict(min_n=-1), dict(min_n=1.5)):
            with pytest.raises(ValueError):
                form(state, flat, good, **kw)
        with pytest.raises(ValueError):
            form(state, flat, dict(good, reserved=[1]))
        with pytest.raises(ValueError):
            form(state, flatten.flat_words((0, 2829), (0, 2829), 1), good)  # 8 003 241 cells
        with pytest.raises(ValueError):
            form(state, dict(flat, l_occ=0), good)


def test_cli_words(sv):
    assert sv.cli_voxel_flatten_spec("-5,45,-20,20,2", 0.2) == ((-5, 45), (-20, 20), 2, 0.2, 2.0)
    assert sv.cli_voxel_flatten_spec("0,8,0,8,4,0.3", 0.2) == ((0, 8), (0, 8), 4, 0.3, 2.0) and sv.cli_voxel_flatten_spec("0,8,0,8,4,0.3,1.5", 0.2)[3:] == (0.3, 1.5)
    assert sv.cli_voxel_flatten_text(range(8)) == "drawn 0, outside 1, below 2, ground 3, obstacle 4, overhead 5, occupied cells 6, free cells 7"
    for bad in ("0,8,0,8", "0,8,0,8,1,0.2,2.0,3", "0,8,0,8,0", "8,0,0,8,1", "0,8,0,8,1.5", "0,8,0,8,1,2.0,2.0", "0,8,0,8,1,nan", "0,3000,0,3000,1", "a,8,0,8,1"):
        with pytest.raises(ValueError):
            sv.cli_voxel_flatten_spec(bad, 0.2)


def _objects(rigmod, case, device, update):
    m = rigmod.VoxelMap(case["params"]["lo"], case["params"]["hi"], case["params"]["size"], case["params"]["capacity"], device=device)
    for call in case["calls"]:
        update(m, call)
    return m


def _host(res):
    return {k: getattr(res, k).cpu().numpy() for k in FIELDS}


def _update_cpu(m, call):
    m.update(*call)


def test_cpu_objects_agree(sv, all_cases, defined):
    """VoxelMap(device="cpu").flatten and OccupancyMap(device="cpu").load_voxels run the numpy form."""
    rigmod = util.pkg("rig")
    c = all_cases["scene"]
    m = _objects(rigmod, c, "cpu", _update_cpu)
    om = rigmod.OccupancyMap(*flatten.SCENE_FLAT, device="cpu")
    assert om.words == c["flat"]
    assert _differ(_host(m.flatten(om)), defined["scene"]) == [] and _differ(_host(m.flatten(om.words)), defined["scene"]) == []
    spec = sv.voxel_flatten_params(m.params, z_ref=0.05, step=0.3, height=1.0, radius=0, min_obstacle=2, min_ground=3)
    want = sv.voxel_map_flatten(_define(sv, c), c["flat"], spec, min_n=1, min_rows=1, since=0)
    got = m.flatten(om, z_ref=0.05, step=0.3, height=1.0, radius=0, min_obstacle=2, min_ground=3)
    assert _differ(_host(got), want) == [] and _differ(want, defined["scene"]) != []
    om.clearance(1.0)
    om.seq = 99
    res = om.load_voxels(m)
    assert _differ(_host(res), defined["scene"]) == [] and res.logodds is om.logodds and res.last_seen is om.last_seen
    assert om.seq == 1 and om._d2 is None and om.clearance_radius is None
    assert np.array_equal(om.state().numpy() == 2, defined["scene"]["cells"][..., 1] >= 1)
    empty = rigmod.VoxelMap(BOX16["lo"], BOX16["hi"], 1.0, 512, device="cpu")
    assert int(om.load_voxels(empty).stats.sum()) == 0 and om.seq == 0 and not om.logodds.any()
    with pytest.raises(ValueError):
        om.load_voxels(defined["scene"])
    with pytest.raises(ValueError):
        m.flatten(om, step=2.0, height=1.0)
    with pytest.raises(TypeError):
        om.load_voxels(m, reach=3)


def _drive(om, height=2.0):
    """clearance -> cost_to_goal -> routes on a loaded map; -> (the field, the route's result, its cells' centres)."""
    om.clearance(2.0)
    field = om.cost_to_goal(flatten.SCENE_GOAL, 0.0)
    res, xy = om.routes(flatten.SCENE_START)
    return field, res, xy


def _check_route(sv, res, xy):
    """The route reaches the goal, passes under the slab and goes round the wall's end."""
    assert res.status.cpu().tolist() == [sv.ROUTE_GOAL]
    way = xy[0, :int(res.length.cpu()[0])]
    assert way[0].tolist() == [1.5, 2.5] and way[-1].tolist() == [14.5, 2.5]
    under = (way[:, 0] > flatten.SCENE_SLAB_X[0]) & (way[:, 0] < flatten.SCENE_SLAB_X[1])
    assert under.sum() >= 3  # the slab's three columns of cells, crossed
    at_wall = (way[:, 0] > flatten.SCENE_WALL_X) & (way[:, 0] < flatten.SCENE_WALL_X + 1)
    assert at_wall.any() and (way[at_wall, 1] > flatten.SCENE_WALL_Y).all()
    assert way[:, 1].max() > flatten.SCENE_WALL_Y > way[0, 1]  # it had to leave its row


def test_the_planner_runs_on_the_loaded_map(sv, all_cases, defined):
    """The slab 3 m above the floor is no obstacle, the wall is: the route from SCENE_START to SCENE_GOAL passes under the one and round
    the other.  With `height` above the slab, the slab closes the map from side to side and there is no route."""
    rigmod = util.pkg("rig")
    c, d = all_cases["scene"], defined["scene"]
    flat = c["flat"]
    slab, wall, beside = _cell(flat, 4.5, 8.5), _cell(flat, 8.5, 3.5), _cell(flat, 8.5, 13.5)
    assert d["cells"][slab].tolist() == [4, 0, 4] and d["logodds"][slab] == -160 and d["cells"][wall].tolist() == [4, 12, 0] and d["logodds"][wall] == 350
    assert d["cells"][beside].tolist() == [4, 0, 0] and d["stats"].tolist() == [1360, 0, 0, 1024, 144, 192, 12, 244]
    m = _objects(rigmod, c, "cpu", _update_cpu)
    om = rigmod.OccupancyMap(*flatten.SCENE_FLAT, device="cpu")
    om.load_voxels(m)
    field, res, xy = _drive(om)
    _check_route(sv, res, xy)
    om.load_voxels(m, height=5.0)
    assert om.logodds[slab] == 4 * 85
    field, res, xy = _drive(om)
    assert res.status.tolist() == [sv.ROUTE_UNREACHABLE] and int(field.cost[_cell(flat, *flatten.SCENE_START)]) == sv.COST_INF


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = {"sv_voxel_flatten_device", "sv_debug_voxel_flatten"}
    assert set(re.findall(r"\(?\b(sv_\w*flatten\w*)\)?\s*\(", src)) == names
    assert text.index("/* ---- (U)") < text.index("/* ---- (V)") < text.index("/* ---- (A)") and " *  (V) " in text
    engine = util.pkg("engine")
    assert set(engine.STAGE_SIGNATURES["voxel_flatten"]) == names and set(engine._GROUP_NEEDS["voxel_flatten"]) == {"voxel_map", "occupancy_map"}
    fields = re.search(r"typedef struct \{([^}]*)\} sv_voxel_flatten_spec;", src).group(1)
    declared = [n.strip().split("[")[0] for part in fields.split(";") if part.strip() for n in part.strip().split(" ", 1)[1].split(",")]
    assert declared == [n for n, _ in engine.SvVoxelFlattenSpec._fields_] and ctypes.sizeof(engine.SvVoxelFlattenSpec) == 64
    assert declared[:7] == list(sv.VOXEL_FLATTEN_WORDS) and len(sv.VOXEL_FLATTEN_STATS) == 8
    build = util.pkg("build")
    assert "voxel_flatten_kernels.hip" in build.SOURCES and "voxel_flatten.cpp" in build.SOURCES and "voxel_flatten_kernels.h" in build.HEADERS
    assert "voxel_map_flatten" in sv.__doc__ and "(V)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_flatten_kernels.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert '#include "voxel_map_table.h"' in source and "asm" not in code and "float" not in code
    # integer atomics only - walk A's two maxima and one minimum, walk B's add and maximum, and one flush of the counters in the walks and
    # in resolve -, none in the floor kernel, and the two maps' own rules: none restated
    assert sorted(re.findall(r"\batomic\w*\(", code)) == ["atomicAdd("] * 3 + ["atomicMax("] * 3 + ["atomicMin("]
    floor_kernel = code[code.index("void k_vflatten_floor"):code.index("void k_vflatten_resolve")]
    assert "atomic" not in floor_kernel and "__shared__" in floor_kernel
    assert code.count("vmap_passes(") == 1 and code.count("vmap_centre(") == 2 and code.count("vmap_zq(") == 1 and code.count("map_cell(") == 1 and code.count("map_grid(") == 2
    assert "65536" not in code and "floor(" not in code.replace("k_vflatten_floor(", "") and "0xFFFFF" not in code
    host = open(os.path.join(build.CSRC, "voxel_flatten.cpp")).read()
    assert "check_voxel_map(" in host and "check_map(" in host and "map_cells_of(" in host and "outputs_overlap(" in host and "hipMalloc" not in host + source
    assert "Synchronize" not in host + source
    for limit in (sv.VOXEL_FLATTEN_CELLS_MAX, sv.COST_CELLS_MAX, sv.FRONTIER_CELLS_MAX):
        assert limit == 8000000
    assert "VFLATTEN_CELLS_MAX = 8000000" in open(os.path.join(build.CSRC, "voxel_flatten_kernels.h")).read()


def _aligned(words, fill, offset_words=0):
    """A host int64 array of `words` words that starts 16-byte aligned plus offset_words words."""
    raw = np.full(words + 3, fill, np.int64)
    skip = ((-raw.ctypes.data) % 16) // 8 + offset_words
    return raw, raw[skip:skip + words]


def test_the_c_entry_refuses(sv, eng):
    """Every check of the C entry runs before any HIP call: host memory stands in for the device buffers, and stays as it was."""
    L = eng.voxel_flatten_lib()
    spec = eng.voxel_map_spec(sv.voxel_map_params(**BOX16))
    need = L.sv_voxel_map_bytes(512)
    rows, cols = 3, 4
    n = rows * cols
    held = {k: _aligned(words, 7)[1] for k, words in (("map", need // 8), ("logodds", n // 4), ("last_seen", n // 2), ("floor", n // 2), ("top", n // 2), ("cells", 3 * n // 2), ("stats", 8))}
    outputs = ("logodds", "last_seen", "floor", "top", "cells", "stats")
    good = dict({k: v.ctypes.data for k, v in held.items()}, map_bytes=need, spec=spec, flat=eng._occupancy_map_struct(flatten.flat_words((0, rows), (0, cols), 1)),
                flatten=eng.voxel_flatten_spec(flatten.words()), min_n=1, min_rows=1, since=0)

    def call(**change):
        a = dict(good, **change)
        ref = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731
        return L.sv_voxel_flatten_device(a["map"], a["map_bytes"], ref(a["spec"]), ref(a["flat"]), ref(a["flatten"]), a["min_n"], a["min_rows"], a["since"],
                                         *(a[k] for k in outputs), None)

    def flat_with(**words):
        return eng._occupancy_map_struct(dict(flatten.flat_words((0, rows), (0, cols), 1), **words))

    def flatten_with(**words):
        s = eng.voxel_flatten_spec(flatten.words())
        for k, v in words.items():
            if k == "reserved":
                s.reserved[v] = 1
            else:
                setattr(s, k, v)
        return s

    def spec_with(**words):
        s = eng.voxel_map_spec(sv.voxel_map_params(**BOX16))
        for k, v in words.items():
            setattr(s, k, v)
        return s

    bad = [(dict(spec=None), b"spec"), (dict(map=None), b"map"), (dict(map=good["map"] + 8), b"map"), (dict(map_bytes=need - 8), b"map"),
           (dict(spec=spec_with(size=0.0)), b"size"), (dict(spec=spec_with(capacity=0)), b"capacity")]
    bad += [(dict(flat=None), b"map spec"), (dict(flat=flat_with(rows=0)), b"rows"), (dict(flat=flat_with(cols=32769)), b"cols"), (dict(flat=flat_with(scale=0)), b"scale"),
            (dict(flat=flat_with(top=1 << 24)), b"top"), (dict(flat=flat_with(l_occ=0)), b"l_occ"), (dict(flat=flat_with(l_min=5)), b"clamp"),
            (dict(flat=flat_with(rows=2829, cols=2829)), b"8 000 000"), (dict(flat=flat_with(rows=32768, cols=32768)), b"8 000 000")]
    bad += [(dict(flatten=None), b"flatten is NULL")] + [(dict(flatten=flatten_with(reserved=k)), b"reserved") for k in (0, 8)]
    bad += [(dict(flatten=flatten_with(**w)), text) for w, text in ((dict(mode=2), b"mode"), (dict(mode=-1), b"mode"), (dict(mode=0, z_ref_q=1 << 30), b"z_ref_q"),
                                                                   (dict(mode=0, z_ref_q=-(1 << 30)), b"z_ref_q"), (dict(step_q=0), b"step_q"), (dict(step_q=1024), b"step_q"),
                                                                   (dict(height_q=1 << 28), b"height_q"), (dict(radius=-1), b"radius"), (dict(radius=9), b"radius"),
                                                                   (dict(min_obstacle=0), b"min_obstacle"), (dict(min_ground=0), b"min_ground"))]
    bad += [(dict(min_n=0), b"min_n"), (dict(min_n=-5), b"min_n")]
    bad += [(dict(**{k: None}), k.encode()) for k in outputs]
    bad += [(dict(stats=good["stats"] + 4), b"8-byte"), (dict(logodds=good["logodds"] + 1), b"2-byte")] + [(dict(**{k: good[k] + 2}), b"4-byte") for k in ("last_seen", "floor", "top", "cells")]
    bad += [(dict(**{k: good["map"] + 64}), b"shares") for k in outputs]
    bad += [(dict(**{b: good[a] + 8}), b"shares") for i, a in enumerate(outputs) for b in outputs[i + 1:]]
    bad += [(dict(logodds=good["cells"] + 12 * n - 2), b"shares"), (dict(stats=good["floor"] - 56), b"shares")]  # the last and the first byte
    for change, text in bad:
        eng.lib().sv_last_error(None)
        assert call(**change) == SV_ERR_ARG, change
        said = eng.lib().sv_last_error(None)
        assert said and said.startswith(b"sv_voxel_flatten") and text in said, (change, said)
    assert all((v == 7).all() for v in held.values())
    assert eng.debug_voxel_flatten(0, 0) == 0 and eng.debug_voxel_flatten(2049, 5) == 0 and eng.debug_voxel_flatten(-1, -1) == 0
    assert eng.debug_voxel_flatten(7, 0) == 0 and eng.debug_voxel_flatten(0, 0) == 7


# ---------------------------------------------------------------------------------------------------------------- GPU

def _engine_map(eng, sv, case):
    words = sv.voxel_map_params(**case["params"])
    buf, seq = eng.voxel_map_new(words), 0
    for call in case["calls"]:
        eng.voxel_map_insert(buf, words, *(None if a is None else _cuda(a) for a in call[:4]), call[4], seq0=seq)
        seq += call[0].shape[0]
    return buf, words


@pytest.mark.gpu
def test_the_device_against_the_numpy_form(sv, eng, all_cases, defined):
    """Every case; then every case again with the table walked by one and by two workgroups, whose lanes make up to sixteen trips."""
    for groups in (0, 1, 2):
        eng.debug_voxel_flatten(groups)
        try:
            for name, case in all_cases.items():
                buf, words = _engine_map(eng, sv, case)
                before = buf.clone()
                got = _host(eng.voxel_map_flatten(buf, words, case["flat"], case["spec"], **case["kw"]))
                assert _differ(got, defined[name]) == [], (groups, name, got["stats"].tolist(), defined[name]["stats"].tolist())
                assert bool((buf == before).all()), name  # the voxel map is only read
        finally:
            assert eng.debug_voxel_flatten(0) == groups


@pytest.mark.gpu
def test_twice_into_the_same_outputs(sv, eng, all_cases, defined):
    """The clear is complete: outputs full of other numbers - an earlier case's, then all ones - come out the same; and `out` is checked."""
    import torch
    first, second = all_cases["shape_9x33"], all_cases["overflowed_local"]  # the same flat shape
    buf, words = _engine_map(eng, sv, first)
    res = eng.voxel_map_flatten(buf, words, first["flat"], first["spec"])
    assert _differ(_host(res), defined["shape_9x33"]) == []
    for spec in (first["spec"], flatten.words(mode=0, z_ref_q=512), flatten.words(radius=0)):
        want = sv.voxel_map_flatten(_define(sv, first), first["flat"], spec)
        for fill in (None, -1, 0x7F7F):
            if fill is not None:
                for k in FIELDS:
                    getattr(res, k).fill_(fill)
            again = eng.voxel_map_flatten(buf, words, first["flat"], spec, out=res)
            assert again.logodds.data_ptr() == res.logodds.data_ptr() and _differ(_host(again), want) == [], (spec, fill)
    other, other_words = _engine_map(eng, sv, second)
    assert _differ(_host(eng.voxel_map_flatten(other, other_words, second["flat"], second["spec"], out=res)), defined["overflowed_local"]) == []
    # z_ref_q is not read in mode 1
    loose = eng.SvVoxelFlattenSpec(mode=1, z_ref_q=1 << 30, step_q=102, height_q=1024, radius=2, min_obstacle=1, min_ground=1)
    flat = eng._occupancy_map_struct(first["flat"])
    vspec = eng.voxel_map_spec(words)
    rc = eng.voxel_flatten_lib().sv_voxel_flatten_device(buf.data_ptr(), buf.numel() * 8, ctypes.byref(vspec), ctypes.byref(flat), ctypes.byref(loose), 1, 1, 0,
                                                         *(getattr(res, k).data_ptr() for k in FIELDS), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and _differ(_host(res), defined["shape_9x33"]) == []
    for kw in (dict(out=eng.VoxelFlattenResult(logodds=torch.zeros((9, 33), dtype=torch.int32, device="cuda"))), dict(out=eng.VoxelFlattenResult(top=torch.zeros((9, 32), dtype=torch.int32, device="cuda"))),
               dict(out=res.logodds), dict(min_n=0), dict(since=2 ** 31)):
        with pytest.raises(ValueError):
            eng.voxel_map_flatten(buf, words, first["flat"], first["spec"], **kw)
    with pytest.raises(ValueError):
        eng.voxel_map_flatten(buf, words, first["flat"], dict(first["spec"], radius=9))
    with pytest.raises(ValueError):
        eng.voxel_map_flatten(buf, words, flatten.flat_words((0, 2829), (0, 2829), 1), first["spec"])


@pytest.mark.gpu
def test_stops_after_a_given_kernel(sv, eng, all_cases, defined):
    """sv_debug_voxel_flatten's second word: after the clear alone the counts are zero and nothing is seen; after walk A `drawn` and
    `outside` stand and the counts are still zero."""
    case, want = all_cases["shape_9x33"], defined["shape_9x33"]
    buf, words = _engine_map(eng, sv, case)
    try:
        eng.debug_voxel_flatten(0, 1)
        got = _host(eng.voxel_map_flatten(buf, words, case["flat"], case["spec"]))
        assert not got["stats"].any() and not got["cells"].any() and (got["last_seen"] == -1).all()
        eng.debug_voxel_flatten(0, 2)
        got = _host(eng.voxel_map_flatten(buf, words, case["flat"], case["spec"]))
        assert got["stats"].tolist() == want["stats"][:2].tolist() + [0] * 6 and not got["cells"].any() and (got["last_seen"] >= 0).sum() == (want["cells"].sum(-1) > 0).sum()
    finally:
        eng.debug_voxel_flatten(0, 0)
    assert _differ(_host(eng.voxel_map_flatten(buf, words, case["flat"], case["spec"])), want) == []


def _update_cuda(m, call):
    m.update(*(None if a is None else _cuda(a) for a in call[:4]), call[4])


@pytest.mark.gpu
def test_carved_pruned_and_recentred_maps(sv, eng):
    """The same life of a map on the device and in numpy - insert, a carve that leaves tombstones, a prune that drops them, a recentre
    after which the spare buffer is the live one -, flattened after every step."""
    rigmod = util.pkg("rig")
    flat = flatten.flat_words((0, 16), (0, 16), 1)
    first = one_frame(cell_points([(8, 8, 4), (3, 8, 4), (8, 8, 0), (3, 8, 0), (12, 3, 1)]))
    second = one_frame(cell_points([(8, 8, 10), (2, 2, 0)]))
    got = {}
    for device, update in (("cuda", _update_cuda), ("cpu", _update_cpu)):
        m = rigmod.VoxelMap(BOX16["lo"], BOX16["hi"], 1.0, 512, device=device)
        for frame in (first, second):
            update(m, frame)
        show = lambda **kw: _host(m.flatten(flat, step=0.6, height=6.0, radius=0, **kw))  # noqa: E731
        steps = [show()]
        xyz, n, counts = ((None if a is None else _cuda(a)) if device == "cuda" else a for a in (second[0], second[2], second[3]))
        res = m.carve(xyz, n, counts, second[4], origin=(8.5, 8.5, 1.5), reach_m=12.0, margin=0, min_miss=1)
        assert (res.stats.cpu().tolist() if device == "cuda" else [res[k] for k in sv.VOXEL_CARVE_STATS])[3] == 1
        steps.append(show())
        m.prune()
        steps.append(show())
        live = m.buffer
        m.recenter(6.0, 6.0)
        assert device == "cpu" or (m.buffer is not live and m._spare is live)  # the spare buffer is the live one now
        steps += [show(), show(since=1)]
        got[device] = steps
    r, c = 16 - 1 - 8, 16 - 1 - 8
    before, carved, pruned, moved, late = got["cpu"]
    assert before["cells"][r, c].tolist() == [1, 1, 1] and carved["cells"][r, c].tolist() == [1, 0, 1] and before["stats"][DRAWN] == carved["stats"][DRAWN] + 1 == 7
    assert _differ(carved, pruned) == [] and moved["stats"][DRAWN] + moved["stats"][OUTSIDE] <= 6 and late["stats"][DRAWN] < moved["stats"][DRAWN]
    assert all(_differ(a, b) == [] for a, b in zip(got["cuda"], got["cpu"]))


@pytest.mark.gpu
def test_end_to_end_on_the_device(sv, eng, all_cases, defined):
    """VoxelMap.update -> carve -> OccupancyMap.load_voxels -> clearance -> cost_to_goal -> frontiers -> routes on the slab-and-wall scene
    with a phantom obstacle that only the first frame saw and the second looked through: every stage's output equals the CPU-tensor
    chain's, and the route is the one the CPU test describes."""
    rigmod = util.pkg("rig")
    c = all_cases["scene"]
    scene = flatten.scene_points()
    phantom = np.array([[12.25, 8.25, 1.1], [12.25, 8.25, 1.6]])
    frames = [one_frame(np.concatenate([scene, phantom])), one_frame(scene)]
    got = {}
    for device, update in (("cuda", _update_cuda), ("cpu", _update_cpu)):
        m = rigmod.VoxelMap(c["params"]["lo"], c["params"]["hi"], c["params"]["size"], c["params"]["capacity"], device=device)
        for frame in frames:
            update(m, frame)
        xyz, n, counts = ((None if a is None else _cuda(a)) if device == "cuda" else a for a in (frames[1][0], frames[1][2], frames[1][3]))
        res = m.carve(xyz, n, counts, frames[1][4], origin=(12.25, 8.25, 5.0), reach_m=12.0, margin=1, min_miss=1)
        carved = (res.stats.cpu().tolist() if device == "cuda" else [res[k] for k in sv.VOXEL_CARVE_STATS])[3]
        om = rigmod.OccupancyMap(*flatten.SCENE_FLAT, device=device)
        loaded = _host(om.load_voxels(m))
        d2 = om.clearance(2.0).cpu().numpy()
        field = om.cost_to_goal(flatten.SCENE_GOAL, 0.0)
        found = om.frontiers(min_cells=1)
        routes, xy = om.routes(flatten.SCENE_START)
        _check_route(sv, routes, xy)
        got[device] = dict(loaded, carved=np.array(carved), seq=np.array(om.seq), d2=d2, cost=field.cost.cpu().numpy(), label=found.label.cpu().numpy(),
                           clusters=found.clusters.cpu().numpy(), info=found.info.cpu().numpy(), route=routes.cells.cpu().numpy(), length=routes.length.cpu().numpy(), xy=xy)
    assert got["cpu"]["carved"] >= 2 and got["cpu"]["seq"] == 2
    at = _cell(c["flat"], 12.25, 8.25)
    assert got["cpu"]["cells"][at].tolist() == [4, 0, 0] and got["cpu"]["logodds"][at] == -160  # the phantom is gone
    assert _differ(got["cpu"], dict(defined["scene"], last_seen=got["cpu"]["last_seen"]), FIELDS) == [] and (got["cpu"]["last_seen"] == 1).all()
    assert [k for k in got["cpu"] if not (got["cuda"][k].shape == got["cpu"][k].shape and got["cuda"][k].dtype == got["cpu"][k].dtype
                                          and got["cuda"][k].tobytes() == got["cpu"][k].tobytes())] == []


@pytest.mark.gpu
def test_cli_voxel_flatten(sv, eng, tmp_path, capsys):
    """--voxel-flatten writes <FILE>.flat.npz at the end of the run, and with --clearance and --goal the planner's outputs on that map.  A
    negative X0 needs the form --voxel-flatten=..., as every option value that starts with a minus sign does."""
    from PIL import Image
    from test_occupancy_map import _drive_frames
    n = 4
    ls, rs = _drive_frames(n)
    for sub in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / sub)
    for i in range(n):
        Image.fromarray(ls[i]).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(rs[i]).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("0.0 0.0 0.0\n0.8 0.05 0.03\n1.6 0.1 0.06\n2.4 0.1 0.09\n")
    full = ["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt")]
    for bad in (full + ["--voxel-flatten=-5,45,-20,20,2"], full + ["--voxel-map", str(tmp_path / "no.ply"), "--voxel-flatten=-5,45,-20,20"],
                full + ["--voxel-map", str(tmp_path / "no.ply"), "--voxel-flatten=-5,45,-20,20,2,3.0"]):
        with pytest.raises(SystemExit):
            sv.main(bad)
    assert not os.path.exists(tmp_path / "no.ply")
    capsys.readouterr()
    sv.main(full + ["--voxel-map", str(tmp_path / "drive.ply"), "--voxel-flatten=-5,45,-20,20,2,0.3", "--occupancy-map", str(tmp_path / "world.png"), "--clearance", "1.0",
                    "--goal", "20,0"])
    said = [line for line in capsys.readouterr().out.splitlines() if line.startswith("voxel map flattened into 100 x 80 cells")]
    assert len(said) == 1
    stats = [int(w.rsplit(" ", 1)[1]) for w in said[0].split(": ")[1].split(", ")]
    got = np.load(tmp_path / "drive.flat.npz")
    assert sorted(got.files) == sorted(["logodds", "last_seen", "floor", "top"] + ["map_" + k for k in sv.OCCUPANCY_MAP_WORDS])  # the word `top` beside the plane `top`
    assert {k: int(got["map_" + k]) for k in sv.OCCUPANCY_MAP_WORDS} == sv.occupancy_map_params((-5, 45), (-20, 20), 2)
    L, seen = got["logodds"], got["last_seen"]
    assert L.shape == seen.shape == got["floor"].shape == got["top"].shape == (100, 80) and L.dtype == np.int16 and seen.dtype == np.int32
    assert stats[0] > 1000 and stats[0] == sum(stats[2:6]) and stats[6] == int((L > 0).sum()) > 10 and stats[7] == int((L < 0).sum()) > 10
    assert ((seen >= 0) == (L != 0)).all() and seen.max() == n - 1 and ((got["floor"] >= 0) >= (seen >= 0)).all()
    assert os.path.exists(tmp_path / "drive.flat.clearance.png") and os.path.exists(tmp_path / "drive.flat.route.txt")
