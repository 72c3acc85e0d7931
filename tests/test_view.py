"""Group (P): the expected view of the world map from candidate poses.  stereo_vision.sv.occupancy_view (with view_rays, view_headings and
view_ranges) is the definition; view_cases.model_view is an independent per-ray model of the same prose; engine.occupancy_view and
rig.OccupancyMap.view / frontier_views must equal the definition in shape, dtype and bits.  The cases of view_cases.py are painted
cell by cell and checked there, on the CPU, against the layouts they name.

Rows of the LDS bitmap hold 2 reach + 1 bits, an odd number: rows of exactly 32 or 64 bits do not exist, so the row lengths tested are
31, 33, 63 and 65 bits - one word, the first bit of a second, the last bit of a second, the first bit of a third."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import map_stage_cases as mc
import util
import view_cases as vc
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from test_occupancy_map import CLI_GRID, _drive_frames, drive  # noqa: F401 (drive: the committed KITTI frames' states, a fixture)
from test_clearance import _fused_recovery_maps

SV_ERR_ARG = -1
KEYS = ("counts", "end_cells", "status", "best", "best_score")
DTYPES = {"counts": np.int32, "end_cells": np.int16, "status": np.uint8, "best": np.int32, "best_score": np.int32}


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _same(got, want):
    """Every array of a view: shape, dtype and bits."""
    return all(_bits(np.asarray(got[k]), want[k]) and want[k].dtype == DTYPES[k] for k in KEYS)


def _differ(got, want):
    return [k for k in KEYS if not _bits(np.asarray(got[k]), want[k])]


@pytest.fixture(scope="module")
def cases(sv):
    """[(case, the definition's result)] of the painted cases - computed once, left unchanged."""
    return [(c, sv.occupancy_view(*vc.args_of(c))) for c in vc.device_cases()]


@pytest.fixture(scope="module")
def random_cases(sv):
    return [(c, sv.occupancy_view(*vc.args_of(c))) for c in vc.random_cases()]


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_hand_case(sv):
    c = vc.hand_case()
    got = sv.occupancy_view(*vc.args_of(c))
    want = {"counts": np.array([[vc.HAND_COUNTS]], np.int32), "end_cells": np.array([[vc.HAND_ENDS]], np.int16), "status": np.array([[vc.HAND_STATUS]], np.uint8),
            "best": np.array([0], np.int32), "best_score": np.array([2], np.int32)}
    assert _same(got, want), _differ(got, want)
    assert _same(vc.model_view(*vc.args_of(c)), want)
    assert (sv.VIEW_FULL, sv.VIEW_HIT, sv.VIEW_EDGE, sv.VIEW_CORNER, sv.VIEW_UNKNOWN, sv.VIEW_INVALID) == (0, 1, 2, 3, 4, 5)
    assert (sv.VIEW_REACH_MAX, sv.VIEW_RAYS_MAX, sv.VIEW_POSES_MAX) == (254, 1024, 65535)
    # the virtual scan: metres between cell centres; the ray that ends in the origin's cell measures 0
    ranges = sv.view_ranges(c["words"], c["poses"], got["end_cells"])
    assert ranges.dtype == np.float64 and ranges.shape == (1, 1, 8) and ranges[0, 0].tolist() == [3.0, 4.0, 4.0, 2.0, math.sqrt(18.0), math.sqrt(2.0), 5.0, 0.0]
    # turned by a quarter: the same fan sees the map to the vehicle's left; (c, s) = (0, 1) is exact
    turned = c["poses"].copy()
    turned[0, 0, 2:] = (0.0, 1.0)
    left = sv.occupancy_view(c["logodds"], c["last_seen"], c["words"], turned, c["ends"][:1], 4, c["occupied"], c["free"])
    assert left["end_cells"][0, 0, 0].tolist() == [3, 1] and left["status"][0, 0, 0] == vc.FULL  # +x of the vehicle is +y of the world: towards lower columns
    # one ray beyond reach is invalid on its own and marks nothing
    short = sv.occupancy_view(c["logodds"], c["last_seen"], c["words"], c["poses"], c["ends"], 3, c["occupied"], c["free"])
    assert short["status"][0, 0].tolist() == [vc.HIT, vc.INVALID, vc.INVALID, vc.HIT, vc.FULL, vc.HIT, vc.INVALID, vc.FULL]
    assert short["end_cells"][0, 0, 1].tolist() == [-1, -1] and short["counts"][0, 0].tolist() == [1, 6, 3]
    lines = sv.view_lines(np.array([[3.5, 4.5, math.pi / 2]]), got["counts"], got["best"], got["best_score"])
    assert lines == ["view 0: heading 90.0 deg, sees 2 unknown, 17 free, 3 occupied cells"]
    assert sv.view_lines(np.zeros((1, 3)), got["counts"], got["best"], np.array([-1])) == ["view 0: no valid pose"]


def test_view_rays_and_headings(sv):
    ends, reach = sv.view_rays(2 * math.pi, 8, 5.0, 10)
    assert ends.dtype == np.float64 and ends.shape == (8, 2) and reach == 51
    angles = np.arctan2(ends[:, 1], ends[:, 0])
    assert np.allclose(np.diff(angles), math.pi / 4) and np.allclose(angles[0], -math.pi + math.pi / 8) and np.allclose(np.hypot(ends[:, 0], ends[:, 1]), 5.0)  # evenly spread
    want, want_reach = vc.fan(2 * math.pi, 8, 5.0, 10)
    assert want_reach == reach and np.allclose(ends, want, rtol=0, atol=1e-12)
    one, reach = sv.view_rays(1.0, 1, 2.5, 2)
    assert one.tolist() == [[2.5, 0.0]] and reach == 6  # a single ray looks straight ahead
    quarter, _ = sv.view_rays(math.pi / 2, 2, 1.0, 1)
    assert np.allclose(quarter, [[math.cos(-math.pi / 8), math.sin(-math.pi / 8)], [math.cos(math.pi / 8), math.sin(math.pi / 8)]])  # the right ray first
    assert sv.view_rays(1.0, 1024, 253.0, 1)[1] == 254 and sv.view_rays(1.0, 3, 25.3, 10)[1] == 254
    for bad in (dict(range_m=253.5), dict(range_m=254.0), dict(range_m=25.31, scale=10), dict(n_rays=0), dict(n_rays=1025), dict(n_rays=2.5), dict(n_rays=True), dict(fov=0.0),
                dict(fov=-1.0), dict(fov=6.3), dict(fov=float("nan")), dict(fov=float("inf")), dict(range_m=float("nan")), dict(range_m=float("inf")), dict(range_m=0.0),
                dict(range_m=-1.0), dict(scale=0), dict(scale=1.5), dict(scale=float("nan"))):
        with pytest.raises(ValueError):
            sv.view_rays(**dict(dict(fov=1.0, n_rays=8, range_m=3.0, scale=1), **bad))
    H = sv.view_headings([[1.0, 2.0], [-3.0, 0.5]], 4)
    assert H.dtype == np.float64 and H.shape == (2, 4, 4)
    assert _bits(H, sv.occupancy_pose(np.array([[1.0], [-3.0]]), np.array([[2.0], [0.5]]), 2 * np.pi * np.arange(4) / 4))
    assert H[1, 0].tolist() == [-3.0, 0.5, 1.0, 0.0] and np.allclose(H[0, 1], [1.0, 2.0, 0.0, 1.0])
    assert sv.view_headings(np.zeros((0, 2)), 16).shape == (0, 16, 4)
    with pytest.raises(ValueError):
        sv.view_headings([[0.0, 0.0]], 0)


def test_definition_equals_the_model_on_random_maps(random_cases):
    kinds = set()
    assert len(random_cases) == 30
    for c, got in random_cases:
        want = vc.model_view(*vc.args_of(c))
        assert _same(got, want), (c["name"], _differ(got, want))
        kinds |= set(np.unique(got["status"]).tolist())
        kinds |= {"no-origin"} if (got["best_score"] < 0).any() else set()
    assert kinds >= {vc.FULL, vc.HIT, vc.EDGE, vc.CORNER, vc.UNKNOWN, vc.INVALID, "no-origin"}  # the random cases reach every way a ray can end


def test_case_layouts_and_the_definition_agree(cases):
    """Every painted case realises the layout it names - under the definition, which equals the model on it."""
    names = [c["name"] for c, _ in cases]
    assert len(names) == len(set(names)) and {n.split("-")[0] for n in names} >= {"directions", "dedup", "rays", "window", "row", "map", "corner", "max", "thresholds", "best", "groups"}
    for c, want in cases:
        assert c["expect"](want), c["name"]
        if c["name"] not in ("groups-2049",):  # the model is a Python loop: the large case is left to the definition
            model = vc.model_view(*vc.args_of(c))
            assert _same(want, model), (c["name"], _differ(want, model))


def test_validation_in_the_definition(sv):
    c = vc.hand_case()
    base = dict(zip(("logodds", "last_seen", "map", "poses", "ends", "reach", "occupied", "free", "max_unknown"), vc.args_of(c)))
    empty = sv.occupancy_view(**dict(base, poses=np.zeros((0, 3, 4))))
    assert empty["counts"].shape == (0, 3, 3) and empty["best"].shape == (0,) and empty["best"].dtype == np.int32 and empty["status"].shape == (0, 3, 8)
    for bad in (dict(reach=0), dict(reach=255), dict(reach=2.5), dict(max_unknown=-1), dict(max_unknown=256), dict(poses=np.zeros((2, 0, 4))), dict(poses=np.zeros((2, 4))),
                dict(poses=np.zeros((256, 256, 4))), dict(poses=np.zeros((1, 1, 3))), dict(ends=np.zeros((0, 2))), dict(ends=np.zeros((1025, 2))), dict(ends=np.zeros((4, 3))),
                dict(logodds=base["logodds"].astype(np.int32)), dict(last_seen=base["last_seen"][:3]), dict(logodds=base["logodds"][:3], last_seen=base["last_seen"][:3]),
                dict(occupied=0.5), dict(free=True), dict(map=dict(base["map"], scale=0)), dict(map=dict(base["map"], rows=0))):
        with pytest.raises(ValueError):
            sv.occupancy_view(**dict(base, **bad))
    assert sv.occupancy_view(**dict(base, poses=np.zeros((65535, 1, 4)) + np.nan, ends=base["ends"][:1]))["best_score"].tolist() == [-1] * 65535


def _c_call(L, base, **kw):
    a = dict(base, **kw)
    return L.sv_view_device(a["logodds"], a["last_seen"], a["map"], a["poses"], a["G"], a["P"], a["ends"], a["n_rays"], a["reach"], a["occupied"], a["free"], a["max_unknown"],
                            a["counts"], a["end_cells"], a["status"], a["best"], a["best_score"], a["ws"], a["ws_bytes"], a["stream"])


def test_validation_needs_no_device(eng):
    """Every SV_ERR_ARG of the C entries, on host buffers, which stay untouched: the checks run before any HIP call."""
    L = eng.view_lib()
    need = ctypes.c_size_t(0)
    assert L.sv_view_workspace(4, 6, ctypes.byref(need)) == 0 and need.value == 32 + 262144  # a byte per cell rounded up to 16, and 65535 scores likewise
    assert L.sv_view_workspace(32768, 32768, ctypes.byref(need)) == 0 and need.value == 2 ** 30 + 262144
    keep = need.value
    for rows, cols, out in ((0, 1, need), (1, 0, need), (32769, 1, need), (1, 32769, need), (-1, 1, need), (4, 6, None)):
        assert L.sv_view_workspace(rows, cols, None if out is None else ctypes.byref(out)) == SV_ERR_ARG and need.value == keep
        assert L.sv_last_error(None).startswith(b"sv_view_workspace")

    names = ("logodds", "last_seen", "poses", "ends", "counts", "end_cells", "status", "best", "best_score")
    bufs = {k: np.full(1024, 0x5A, np.uint8) for k in names}
    bufs["ws"] = np.full(32 + 262144 + 32, 0x5A, np.uint8)
    ptr = lambda name: bufs[name].ctypes.data + (-bufs[name].ctypes.data) % 16  # noqa: E731
    spec = lambda **kw: ctypes.byref(eng._occupancy_map_struct(dict(vc.words_of(4, 6), **kw)))  # noqa: E731
    base = dict({k: ptr(k) for k in names}, map=spec(), G=2, P=3, n_rays=5, reach=4, occupied=85, free=-40, max_unknown=0, ws=ptr("ws"), ws_bytes=32 + 262144, stream=None)
    assert eng.debug_view(0, 3) == 0
    bad = [dict(logodds=None), dict(last_seen=None), dict(ends=None), dict(ws=None), dict(poses=None), dict(counts=None), dict(end_cells=None), dict(status=None), dict(best=None),
           dict(best_score=None), dict(map=None),
           dict(logodds=ptr("logodds") + 1), dict(last_seen=ptr("last_seen") + 2), dict(poses=ptr("poses") + 4), dict(ends=ptr("ends") + 4), dict(counts=ptr("counts") + 2),
           dict(end_cells=ptr("end_cells") + 2), dict(best=ptr("best") + 1), dict(best_score=ptr("best_score") + 2), dict(ws=ptr("ws") + 8),
           dict(reach=0), dict(reach=255), dict(reach=-1), dict(n_rays=0), dict(n_rays=1025), dict(G=-1), dict(G=21846), dict(G=65535, P=2), dict(G=2 ** 30, P=4), dict(P=0),
           dict(P=-1), dict(G=0, P=0), dict(max_unknown=-1), dict(max_unknown=256),
           dict(map=spec(rows=0)), dict(map=spec(cols=32769)), dict(map=spec(scale=0)), dict(map=spec(top=1 << 24)), dict(map=spec(l_occ=0)), dict(map=spec(l_min=1)),
           dict(ws_bytes=32 + 262144 - 1), dict(ws_bytes=0),
           # an output over an input, over another output, over the workspace
           dict(counts=ptr("logodds") + 44), dict(status=ptr("last_seen") + 92), dict(end_cells=ptr("poses") + 188), dict(best=ptr("ends") + 76), dict(end_cells=ptr("counts") + 68),
           dict(status=ptr("end_cells") + 116), dict(best=ptr("status") + 28), dict(best_score=ptr("best") + 4), dict(counts=ptr("ws") + 262144), dict(ws=ptr("best_score") - 262144 - 32 + 16)]
    for kw in bad:
        rc, text = _c_call(L, base, **kw), L.sv_last_error(None)
        assert rc == SV_ERR_ARG and text and text.startswith(b"sv_view:"), (sorted(kw), rc, text)
    # no group: nothing to do, whatever the candidates' pointers are
    assert _c_call(L, base, G=0) == 0 and _c_call(L, base, G=0, poses=None, counts=None, end_cells=None, status=None, best=None, best_score=None) == 0
    assert all((b == 0x5A).all() for b in bufs.values())
    for variant, stages in ((-1, 3), (2, 3), (0, 0), (0, 4)):
        assert eng.debug_view(variant, stages) == SV_ERR_ARG and L.sv_last_error(None).startswith(b"sv_debug_view")
    assert eng.debug_view(0, 3) == 0


def test_header_build_and_loader_agree(eng):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = {n for n in re.findall(r"\b(sv_[a-z_]*view[a-z_]*)\s*\(", src) if "top_view" not in n}  # group (D) is the top view
    assert declared == {"sv_view_workspace", "sv_view_device", "sv_debug_view"}
    assert text.index("/* ---- (O)") < text.index("/* ---- (P)") < text.index("/* ---- (A)")
    L = eng.view_lib()
    assert all(hasattr(L, n) for n in declared) and len(L.sv_view_device.argtypes) == 20
    assert set(eng.STAGE_SIGNATURES["view"]) == declared and eng._GROUP_NEEDS["view"] == ("occupancy_map",)
    build = util.pkg("build")
    assert "view_kernels.hip" in build.SOURCES and "view.cpp" in build.SOURCES and "view_kernels.h" in build.HEADERS
    assert all(os.path.exists(os.path.join(build.CSRC, n)) for n in ("view_kernels.hip", "view.cpp", "view_kernels.h"))
    mc.check_map_cells(build)  # the cell rules the map's readers share are defined once
    sv_mod = util.pkg("stereo_vision.sv")
    assert all(n in sv_mod.__doc__ for n in ("view_rays", "view_headings", "occupancy_view", "view_ranges")) and "(P)" in sv_mod.__doc__


def _arrive(world):
    """frontiers -> frontier_views on the recovery scene -> (goals, poses, the result's arrays, a plain view's arrays)."""
    world.clearance(1.0)
    world.cost_to_goal((12.0, 0.0), 0.5)
    found = world.frontiers(min_cells=1)
    goals = world.frontier_goals(found)
    poses, res = world.frontier_views(found, headings=8, fov=math.pi / 2, range_m=6.0, n_rays=48, max_unknown=3)
    arrays = {k: getattr(res, k).cpu().numpy().copy() for k in KEYS}
    plain = world.view(np.array([[3.25, -1.5, 0.3], [3.25, -1.5, 2.0], [500.0, 0.0, 0.0]]), 2 * math.pi, 8.0, n_rays=96)
    return goals, poses, arrays, {k: getattr(plain, k).cpu().numpy().copy() for k in KEYS}


def test_map_class_on_cpu_tensors(sv):
    """rig.OccupancyMap.view / frontier_views on CPU tensors run the numpy definitions: the end of the exploration loop without a GPU."""
    import torch
    (world,) = _fused_recovery_maps(sv, ["cpu"])
    with pytest.raises(ValueError):
        world.frontier_views()  # no frontiers yet
    goals, poses, got, plain = _arrive(world)
    n = len(goals)
    assert n == 4 and poses.shape == (n, 3) and poses.dtype == np.float64 and got["counts"].shape == (n, 8, 3) and got["status"].shape == (n, 8, 48)
    window = sv.view_headings(goals, 8)
    ends, reach = sv.view_rays(math.pi / 2, 48, 6.0, world.words["scale"])
    want = sv.occupancy_view(world.logodds.numpy(), world.last_seen.numpy(), world.words, window, ends, reach, 85, -40, 3)
    assert _same(got, want), _differ(got, want)
    yaws = 2 * np.pi * np.arange(8) / 8
    assert np.array_equal(poses, np.stack([goals[:, 0], goals[:, 1], yaws[want["best"]]], 1))  # window[best], as (x, y, yaw)
    assert (want["best_score"] > 0).all() and (want["counts"][..., 0].max(1) == want["best_score"]).all()  # a frontier's goal sees undecided cells
    assert isinstance(world._view, util.pkg("engine").ViewResult) and world._view.status.dtype == torch.uint8 and world._view.end_cells.dtype == torch.int16
    # [K, 3] is K groups of one candidate; the third stands outside the map
    assert plain["counts"].shape == (3, 1, 3) and plain["best"].tolist() == [0, 0, 0] and plain["best_score"][2] == -1 and plain["best_score"][0] > 0
    assert (plain["status"][2] == vc.INVALID).all() and not (plain["status"][:2] == vc.INVALID).any()
    ranges = sv.view_ranges(world.words, sv.occupancy_pose([3.25, 3.25, 500.0], [-1.5, -1.5, 0.0], [0.3, 2.0, 0.0])[:, None], plain["end_cells"])
    assert ranges.shape == (3, 1, 96) and np.isnan(ranges[2]).all() and np.nanmax(ranges[:2]) <= 8.0 + 2 * math.sqrt(2) / world.words["scale"] and np.nanmin(ranges[:2]) >= 0.0
    four = world.view(sv.occupancy_pose([3.25], [-1.5], [0.3])[None], 2 * math.pi, 8.0, n_rays=96)  # [G, P, 4]
    assert _bits(four.counts.numpy()[0, 0], plain["counts"][0, 0])
    for bad in (dict(poses=np.zeros((3,))), dict(poses=np.zeros((2, 2, 2, 3))), dict(poses=np.zeros((2, 5))), dict(fov=0.0), dict(range_m=300.0), dict(n_rays=0)):
        with pytest.raises(ValueError):
            world.view(**dict(dict(poses=np.zeros((2, 3)), fov=1.0, range_m=5.0), **bad))


# ---------------------------------------------------------------------------------------------------------------- GPU

def _view_gpu(eng, c, **kw):
    res = eng.occupancy_view(_cuda(c["logodds"]), _cuda(c["last_seen"]), c["words"], c["poses"], c["ends"], c["reach"], c["occupied"], c["free"], c["max_unknown"], **kw)
    return res, {k: getattr(res, k).cpu().numpy() for k in KEYS}


@pytest.fixture()
def variant(eng):
    """Sets sv_debug_view for a test and puts the default back."""
    import torch

    def choose(v, stages=3):
        torch.cuda.synchronize()
        assert eng.debug_view(v, stages) == 0
    yield choose
    torch.cuda.synchronize()
    assert eng.debug_view(0, 3) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", (0, 1))
def test_device_equals_the_definition(eng, cases, variant, which):
    """Every painted case, with the LDS window sized by reach and always 509 cells a side: counts, end cells, status and the best."""
    variant(which)
    wrong = []
    for c, want in cases:
        _, got = _view_gpu(eng, c)
        if not _same(got, want):
            wrong.append((c["name"], _differ(got, want), got["counts"].reshape(-1, 3)[:2].tolist(), want["counts"].reshape(-1, 3)[:2].tolist()))
    assert not wrong, wrong


@pytest.mark.gpu
def test_random_maps_on_the_device(eng, random_cases):
    wrong = []
    for c, want in random_cases:
        _, got = _view_gpu(eng, c)
        if not _same(got, want):
            wrong.append((c["name"], _differ(got, want)))
    assert not wrong, wrong


@pytest.mark.gpu
def test_mechanics(sv, eng, cases):
    """No group at all, out= and the workspace reused across two cases, a misaligned map, a stream of its own, tensors for poses and ends,
    and refusals that enqueue nothing."""
    import torch
    by_name = {c["name"]: (c, want) for c, want in cases}
    first = by_name["rays-257"]
    res, got = _view_gpu(eng, first[0])
    assert _same(got, first[1]) and res.workspace.numel() == 1600 + 262144
    # G = 0: nothing written, nothing enqueued
    c = first[0]
    none = eng.occupancy_view(_cuda(c["logodds"]), _cuda(c["last_seen"]), c["words"], np.zeros((0, 3, 4)), c["ends"], c["reach"], 85, -40)
    assert none.counts.shape == (0, 3, 3) and none.end_cells.shape == (0, 3, 257, 2) and none.best.shape == (0,)
    # the same shapes again, into the first call's tensors, from other poses: nothing stale may stay
    moved = dict(c, poses=c["poses"][:, ::-1].copy())
    again = eng.occupancy_view(_cuda(c["logodds"]), _cuda(c["last_seen"]), c["words"], torch.from_numpy(moved["poses"]).cuda(), torch.from_numpy(c["ends"]).cuda(), c["reach"], 85, -40,
                               out=res, workspace=res.workspace)
    assert again.counts is res.counts and again.status is res.status and again.workspace is res.workspace
    assert _same({k: getattr(again, k).cpu().numpy() for k in KEYS}, sv.occupancy_view(*vc.args_of(moved)))
    # a map that starts 2 bytes into its storage: the state kernel's cell-by-cell path
    store_l, store_s = torch.zeros(1601, dtype=torch.int16, device="cuda"), torch.zeros(1601, dtype=torch.int32, device="cuda")
    L, S = store_l[1:].view(40, 40), store_s[1:].view(40, 40)
    L.copy_(_cuda(c["logodds"])), S.copy_(_cuda(c["last_seen"]))
    assert L.data_ptr() % 16 != 0
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        off = eng.occupancy_view(L, S, c["words"], c["poses"], c["ends"], c["reach"], 85, -40, out=(res.counts, res.end_cells, res.status, res.best, res.best_score))
    stream.synchronize()
    assert _same({k: getattr(off, k).cpu().numpy() for k in KEYS}, first[1])
    # refused: the outputs keep their bytes
    marks = [torch.full_like(getattr(res, k), 77) for k in KEYS]
    small = torch.empty(res.workspace.numel() - 1, dtype=torch.uint8, device="cuda")
    good = dict(logodds=_cuda(c["logodds"]), last_seen=_cuda(c["last_seen"]), map=c["words"], poses=c["poses"], ends=c["ends"], reach=c["reach"], occupied=85, free=-40, out=tuple(marks))
    for bad in (dict(reach=0), dict(reach=255), dict(max_unknown=256), dict(workspace=small), dict(out=tuple(marks[:4])), dict(out=(marks[0].view(-1),) + tuple(marks[1:])),
                dict(out=(marks[0], marks[1].int(), marks[2], marks[3], marks[4])), dict(logodds=good["logodds"].cpu()), dict(last_seen=good["last_seen"].long()),
                dict(logodds=good["logodds"][:39]), dict(poses=np.zeros((1, 0, 4))), dict(poses=np.zeros((300, 300, 4))), dict(ends=np.zeros((1025, 2))), dict(ends=np.zeros((0, 2))),
                dict(map=dict(c["words"], rows=39))):
        with pytest.raises(ValueError):
            eng.occupancy_view(**dict(good, **bad))
    torch.cuda.synchronize()
    assert all((m == 77).all().item() for m in marks)


@pytest.mark.gpu
def test_map_class_on_the_device(sv, eng, drive):
    """rig.OccupancyMap.view / frontier_views on the device against the class on CPU tensors on the recovery scene; and the committed
    drive's map against the numpy form."""
    world, cpu = _fused_recovery_maps(sv, ["cuda", "cpu"])
    (goals, poses, got, plain), (goals_cpu, poses_cpu, want, plain_cpu) = _arrive(world), _arrive(cpu)
    assert _bits(goals, goals_cpu) and _bits(poses, poses_cpu) and len(goals) == 4
    assert _same(got, want), _differ(got, want)
    assert _same(plain, plain_cpu), _differ(plain, plain_cpu)
    window = sv.view_headings(goals, 8)
    yaws = 2 * np.pi * np.arange(8) / 8
    for k in range(len(goals)):  # the returned pose is window[best]
        assert _bits(sv.occupancy_pose(*poses[k]), window[k, got["best"][k]]) and poses[k, 2] == yaws[got["best"][k]]
    held = world._view
    assert held.counts.is_cuda and held.workspace is not None
    again = world.view(np.array([[3.25, -1.5, 0.3], [3.25, -1.5, 2.0], [500.0, 0.0, 0.0]]), 2 * math.pi, 8.0, n_rays=96)
    assert again.counts is held.counts and again.workspace is held.workspace  # the tensors stay with the map

    _, _, _, words, fused = drive
    logodds, last_seen = fused["logodds"], fused["last_seen"]
    ends, reach = sv.view_rays(math.pi / 2, 128, 12.0, words["scale"])
    Xw, Yw = sv.occupancy_map_centres(words)
    at = sv.view_headings(np.stack([Xw[::max(1, len(Xw) // 5)][:5], Yw[len(Yw) // 2] + 0 * Xw[:5]], 1), 6)
    want = sv.occupancy_view(logodds, last_seen, words, at, ends, reach, 85, -40, 4)
    res = eng.occupancy_view(_cuda(logodds), _cuda(last_seen), words, at, ends, reach, 85, -40, 4)
    assert _same({k: getattr(res, k).cpu().numpy() for k in KEYS}, want) and want["counts"].sum() > 1000


@pytest.mark.gpu
def test_cli_prints_the_best_heading_per_frontier(sv, eng, drive, tmp_path, capsys):
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
    common = ["-k", str(tmp_path / "kitti"), "--batch", "2", "--occupancy-map", out, "--poses", str(tmp_path / "poses.txt"), "--clearance", "1.0"]
    for bad in (["--view", "90,8"], ["--frontiers", "3", "--view", "90"], ["--frontiers", "3", "--view", "0,8"], ["--frontiers", "3", "--view", "90,26"],
                ["--frontiers", "3", "--view", "90,8,0"], ["--frontiers", "3", "--view", "90,8,64,0"], ["--frontiers", "3", "--view", "90,8,64,8,1"], ["--frontiers", "3", "--view", "x,8"]):
        with pytest.raises(SystemExit):
            sv.main(common + bad)
    assert not os.path.exists(out)
    ranges = sv.occupancy_map_cover(xyyaw, sv.CLI_TOP_VIEW["x_range"], sv.CLI_TOP_VIEW["y_range"])
    cpu = util.pkg("rig").OccupancyMap(ranges[0], ranges[1], 10, device="cpu")
    cpu.update(states[:2], sv.occupancy_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2]), CLI_GRID)
    cpu.clearance(1.0)
    cpu.cost_to_goal(xyyaw[-1, :2], 1.0)
    found = cpu.frontiers(min_cells=3)
    poses, seen = cpu.frontier_views(found, headings=12, fov=math.radians(90.0), range_m=8.0, n_rays=64)
    lines = sv.view_lines(poses, seen.counts.numpy(), seen.best.numpy(), seen.best_score.numpy())
    assert len(lines) == int(found.info[3]) >= 1 and lines[0].startswith("view 0: heading ")
    capsys.readouterr()
    sv.main(common + ["--frontiers", "3", "--view", "90,8,64,12"])
    printed = capsys.readouterr().out
    assert "".join(line + "\n" for line in lines) in printed
