"""The connected components of the voxel map (group (W)): stereo_vision.sv.voxel_map_clusters against its flood-fill form and hand
numbers, and engine.voxel_map_clusters / rig.VoxelMap.clusters / .despeckle against the definition.  Every comparison is shape, dtype and
bytes."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
import voxel_cluster_cases as cluster
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_map_cases import BOX16, cell_points, one_frame

SV_ERR_ARG = -1
FIELDS = ("clusters", "info", "key", "label")
MEMBERS, COMPONENTS, KEPT, SMALL, EMPTIED, LARGEST = range(6)


def _differ(got, want, fields=FIELDS):
    return [k for k in fields if not (got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes())]


def _define(sv, case):
    """The numpy state of a case after its ops."""
    state, seq = sv.voxel_map_state(sv.voxel_map_params(**case["params"])), 0
    for op in case["ops"]:
        if op[0] == "update":
            sv.voxel_map_insert(state, *op[1], seq0=seq)
            seq += op[1][0].shape[0]
        else:
            xyz, _, n, counts, poses = op[1]
            sv.voxel_map_carve(state, xyz, n, counts, poses, **op[2])
    return state


def _floor(sv, case, state):
    """(the flat map's words, the flatten's floor plane) of a mode 1 case, else (None, None)."""
    if case["flat"] is None:
        return None, None
    return case["flat"]["map"], sv.voxel_map_flatten(state, case["flat"]["map"], case["flat"]["flatten"], **case["kw"])["floor"]


def _clusters(sv, case, form=None):
    state = _define(sv, case)
    return (form or sv.voxel_map_clusters)(state, case["spec"], *_floor(sv, case, state), **case["kw"]), state


@pytest.fixture(scope="module")
def all_cases(sv):
    return cluster.all_cases(sv.voxel_map_slot_of)


@pytest.fixture(scope="module")
def defined(sv, all_cases):
    """Per case the numpy form's result, computed once and left as it is."""
    return {name: _clusters(sv, c)[0] for name, c in all_cases.items()}


def _key(cell):
    return int(cell[0]) | int(cell[1]) << 20 | int(cell[2]) << 40


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_vectorised_against_brute(sv, all_cases, defined):
    for name, c in all_cases.items():
        brute, _ = _clusters(sv, c, sv.voxel_map_clusters_brute)
        assert _differ(defined[name], brute) == [], (name, defined[name]["info"].tolist(), brute["info"].tolist())


def test_hand_numbers(sv, all_cases, defined):
    """The sizes case by hand: lines of 3, 4 and 5 voxels along axis 0 with the weights 1 .. 12 in that order, min_voxels 4.  And the band:
    of six voxels with zq = 128 + 256 z over z_ref_q = 100 the band 284 <= h < 1052 takes z = 1, 2, 3."""
    d = defined["sizes_keep"]
    assert d["info"].tolist() == [12, 3, 2, 3, 0, 5, 0, 0]
    four = [_key((1, 6, 2)), 4, 4 + 5 + 6 + 7, 1, 6, 2, 4, 6, 2, (1 + 2 + 3 + 4) * 256 + 4 * 128, 4 * (6 * 256 + 128), 4 * (2 * 256 + 128), 0, 0, 4, 0]
    five = [_key((1, 10, 2)), 5, 8 + 9 + 10 + 11 + 12, 1, 10, 2, 5, 10, 2, (1 + 2 + 3 + 4 + 5) * 256 + 5 * 128, 5 * (10 * 256 + 128), 5 * (2 * 256 + 128), 0, 0, 5, 0]
    assert d["clusters"].tolist() == [four, five] and d["clusters"].dtype == np.int64
    assert d["label"].tolist() == [-2] * 3 + [0] * 4 + [1] * 5 and d["label"].dtype == np.int32 and d["key"].tolist() == sorted(d["key"].tolist())
    boxes = sv.voxel_cluster_boxes(d["clusters"], BOX16)
    assert boxes["centre"].tolist() == [[3.0, 6.5, 2.5], [3.5, 10.5, 2.5]] and boxes["lo"].tolist() == [[1.0, 6.0, 2.0], [1.0, 10.0, 2.0]]
    assert boxes["hi"].tolist() == [[5.0, 7.0, 3.0], [6.0, 11.0, 3.0]] and boxes["voxels"].tolist() == [4, 5] and boxes["centre"].dtype == np.float64
    b = defined["band"]
    assert b["info"][:6].tolist() == [3, 1, 1, 0, 0, 3] and b["label"].tolist() == [-1, 0, 0, 0, -1, -1]
    assert b["clusters"][0, :9].tolist() == [_key((8, 8, 1)), 3, 3, 8, 8, 1, 8, 8, 3] and b["clusters"][0, 11] == 3 * 128 + (1 + 2 + 3) * 256


def test_the_cases_show_what_they_are_for(sv, all_cases, defined):
    d = defined
    for how, counts in cluster.TOUCH_COMPONENTS.items():
        assert tuple(int(d["touch_%s_%d" % (how, conn)]["info"][COMPONENTS]) for conn in (6, 18, 26)) == counts, how
    # the wrap: the key one below a cell's is a voxel of the map, on the far side of the box, and the two are no neighbours
    n = cluster.WRAP_CELLS
    assert n == 2 ** 20 == sv.VOXEL_CELLS_MAX
    for name, here, there, comps in (("wrap_x", (0, 5, 5), (n - 1, 4, 5), 6), ("wrap_y", (7, 0, 5), (7, n - 1, 4), 4)):
        state = _define(sv, all_cases[name])
        assert n in state["params"]["cells"] and {_key(here), _key(there)} <= set(state["key"].tolist())
        assert _key(here) - (1 if name == "wrap_x" else 1 << 20) == _key(there)
        assert d[name]["info"][:3].tolist() == [comps] * 3 and d[name]["info"][LARGEST] == 1, name  # every voxel alone: the axes' ends are no neighbours either
    # the tombstone keeps its key, is no member and cuts the line
    for name in ("tombstone_carved", "tombstone_min_n"):
        got = d[name]
        assert got["key"].tolist() == [_key(c) for c in cluster.LINE] and got["label"].tolist() == [0, -1, 1] and got["info"][:3].tolist() == [2, 2, 2], name
    state = _define(sv, all_cases["tombstone_carved"])
    assert state["n"].tolist() == [5, 0, 5] and len(state["key"]) == 3
    assert _define(sv, all_cases["tombstone_min_n"])["n"].tolist() == [5, 1, 5]
    # the probe: four keys that start at slot 1022 of 1024
    state = _define(sv, all_cases["probe"])
    starts = sv.voxel_map_slot_of(state["key"], 1024)
    assert (starts == cluster.PROBE_SLOT).sum() >= 3 and d["probe"]["info"][COMPONENTS] == (starts == cluster.PROBE_SLOT).sum() and d["probe"]["info"][LARGEST] == 2
    # the schedule: one set of voxels, one result
    order, back, mixed = (all_cases["schedule_" + k]["ops"][0][1][0][0] for k in ("in_order", "reversed", "shuffled"))
    assert order.tolist() == back[::-1].tolist() and order.tolist() != mixed[:300].tolist() and mixed.shape[0] == 337
    assert _differ(d["schedule_in_order"], d["schedule_reversed"]) == [] and _differ(d["schedule_in_order"], d["schedule_shuffled"]) == []
    assert d["schedule_in_order"]["info"][COMPONENTS] > 5 and d["schedule_in_order"]["info"][LARGEST] > 64
    # the snake: a 6-connected path, every step one cell on one axis
    path = np.array(cluster.snake_path())
    assert len(path) >= 400 and len(set(map(tuple, path))) == len(path) and (np.abs(np.diff(path, axis=0)).sum(1) == 1).all()
    for name in ("snake_forward", "snake_backward"):
        assert d[name]["info"][:6].tolist() == [len(path), 1, 1, 0, 0, len(path)], name
    assert _differ(d["snake_forward"], d["snake_backward"]) == []
    assert d["snake_every_second"]["info"][:3].tolist() == [(len(path) + 1) // 2] * 3 and d["snake_every_second"]["info"][LARGEST] == 1
    assert d["slab"]["info"][:6].tolist() == [512, 1, 1, 0, 0, 512] and all_cases["slab"]["params"]["capacity"] == 512
    # sizes: k - 1, k and k + 1 voxels at min_voxels = k
    k = cluster.SIZES_K
    assert sorted(cluster.SIZES_LINES) == [k - 1, k, k + 1] and d["sizes_keep"]["clusters"][:, 1].tolist() == [k, k + 1]
    assert d["sizes_drop"]["info"].tolist() == [12, 3, 2, k - 1, k - 1, k + 1, 0, 0] and _differ(d["sizes_keep"], d["sizes_drop"]) == ["info"]
    # capacity: 70 kept, 64 rows - the 64 least keys -, six components cut
    got = d["capacity"]
    keys = np.sort(_define(sv, all_cases["capacity"])["key"])
    assert got["info"][:3].tolist() == [70, 70, 70] and got["clusters"].shape == (64, 16) and got["clusters"][:, 0].tolist() == keys[:64].tolist()
    assert got["label"].tolist() == list(range(64)) + [-3] * 6
    # the floor: one piece with the ground, three without it, and those are the flatten's obstacle voxels inside the flat map
    one, three = d["floor_all_heights"], d["floor_over_the_floor"]
    c = all_cases["floor_over_the_floor"]
    flat = sv.voxel_map_flatten(_define(sv, c), c["flat"]["map"], c["flat"]["flatten"])
    assert one["info"][:6].tolist() == [272, 1, 1, 0, 0, 272]
    assert three["info"][:3].tolist() == [flat["stats"][4], 3, 3] and sorted(three["clusters"][:, 1].tolist()) == [3, 3, 8] and flat["stats"][1] > 0
    outside = [_key(cluster.FLOOR_OUTSIDE + (z,)) for z in (1, 2)]
    assert all(three["label"][three["key"].tolist().index(key)] == -1 for key in outside)
    assert d["empty"]["info"].tolist() == [0] * 8 and d["empty"]["clusters"].shape == (0, 16) and d["empty"]["label"].shape == (0,)
    assert d["overflowed"]["info"].tolist() == [-1] + [0] * 7 and d["overflowed"]["label"].tolist() == [-1, -1] and d["overflowed"]["clusters"].shape == (0, 16)


def test_params_and_refusals(sv):
    p = sv.voxel_map_params(lo=(0.0, 0.0, -1.0), hi=(16.0, 16.0, 7.0), size=0.5, capacity=512)
    assert sv.voxel_cluster_params(p) == dict(connectivity=26, mode=0, z_ref_q=0, h_lo_q=-2 ** 30, h_hi_q=2 ** 30, min_voxels=1, capacity=1024, drop=0)
    assert sv.voxel_cluster_params(p, 6, 5, 9, 0, 0.0, 0.2, 2.0, True) == dict(connectivity=6, mode=0, z_ref_q=512, h_lo_q=102, h_hi_q=1024, min_voxels=5, capacity=9, drop=1)
    assert sv.voxel_cluster_params(p, mode=1, z_ref=3.0) == dict(connectivity=26, mode=1, z_ref_q=0, h_lo_q=102, h_hi_q=1024, min_voxels=1, capacity=1024, drop=0)
    assert sv.voxel_cluster_params(p, mode=1, h_lo=-0.5, h_hi=0.5)["h_lo_q"] == -256
    assert list(sv.voxel_cluster_params(p)) == list(sv.VOXEL_CLUSTER_WORDS) and len(sv.VOXEL_CLUSTER_ROW) == 16 and len(sv.VOXEL_CLUSTER_OFFSETS) == 13
    assert sorted(sum(v != 0 for v in o) for o in sv.VOXEL_CLUSTER_OFFSETS) == [1] * 3 + [2] * 6 + [3] * 4
    assert all((o[2], o[1], o[0]) < (0, 0, 0) for o in sv.VOXEL_CLUSTER_OFFSETS)
    for bad in (dict(connectivity=8), dict(connectivity=True), dict(mode=2), dict(min_voxels=0), dict(capacity=0), dict(capacity=65536), dict(drop=2), dict(h_lo=2.0, h_hi=2.0),
                dict(h_lo=3.0, h_hi=1.0), dict(h_lo=float("nan")), dict(z_ref=float("inf")), dict(z_ref="a"), dict(h_hi=1e12), dict(min_voxels=2.5)):
        with pytest.raises(ValueError):
            sv.voxel_cluster_params(p, **bad)
    good = sv.voxel_cluster_params(p)
    for bad in (dict(z_ref_q=2 ** 30 + 1), dict(h_lo_q=-2 ** 30 - 1), dict(h_hi_q=2 ** 30 + 1), dict(h_lo_q=5, h_hi_q=5), dict(reserved=[0, 1]), dict(connectivity=None)):
        with pytest.raises(ValueError):
            sv.voxel_cluster_words(dict(good, **bad))
    state = sv.voxel_map_state(sv.voxel_map_params(**BOX16))
    for kw in (dict(min_n=0), dict(min_n=True)):
        with pytest.raises(ValueError):
            sv.voxel_map_clusters(state, cluster.words(), **kw)
    flat = cluster.flat_words((0, 4), (0, 4), 1)
    for args in ((None, None), (flat, None), (flat, np.zeros((4, 4), np.int64)), (flat, np.zeros((4, 5), np.int32))):
        with pytest.raises(ValueError):
            sv.voxel_map_clusters(state, cluster.words(mode=1), *args)


def test_cli_words(sv):
    assert sv.cli_voxel_clusters_spec("20", 0.2) == (20, 26, None, None) and sv.cli_voxel_clusters_spec("5,6", 0.2) == (5, 6, None, None)
    assert sv.cli_voxel_clusters_spec("5,18,0.3,2.5", 0.2) == (5, 18, 0.3, 2.5)
    for bad in ("", "0", "5,7", "5,6,0.3", "5,6,0.3,2.5,1", "5,6,2.5,0.3", "a", "5,6,nan,1", "2.5"):
        with pytest.raises(ValueError):
            sv.cli_voxel_clusters_spec(bad, 0.2)
    boxes = sv.voxel_cluster_boxes(np.array([[7, 2, 9, 1, 2, 3, 2, 2, 3, 768, 1280, 1792, 4, 5, 2, 0]]), BOX16)
    assert sv.cli_voxel_cluster_lines(boxes) == ["7 2 1.5 2.5 3.5 1.0 2.0 3.0 3.0 3.0 4.0 4 5"]
    colors = sv.voxel_cluster_colors(np.arange(100))
    assert colors.shape == (100, 4) and colors.dtype == np.uint8 and (colors[:, :3] >= 64).all() and len(set(map(tuple, colors.tolist()))) > 90


def _objects(rigmod, case, device, to):
    """A VoxelMap on `device` after the case's ops; to: a host array's way onto the device."""
    p = case["params"]
    m = rigmod.VoxelMap(p["lo"], p["hi"], p["size"], p["capacity"], device=device)
    for op in case["ops"]:
        xyz, color, n, counts, poses = op[1]
        if op[0] == "update":
            m.update(*(None if a is None else to(a) for a in (xyz, color, n, counts)), poses)
        else:
            kw = dict(op[2])
            m.carve(to(xyz), None if n is None else to(n), to(counts), poses, reach_m=float(kw.pop("reach")) * p["size"], **kw)
    return m


def _object_clusters(rigmod, case, m, **more):
    """m.clusters for the case's words, over the case's own flatten in mode 1."""
    s = case["spec"]
    size, lo_z = case["params"]["size"], case["params"]["lo"][2]
    kw = dict(connectivity=s["connectivity"], min_voxels=s["min_voxels"], capacity=s["capacity"], drop=bool(s["drop"]), **case["kw"])
    if s["mode"] == 1:
        f = case["flat"]["flatten"]
        res = m.flatten(case["flat"]["map"], step=f["step_q"] * size / 256, height=f["height_q"] * size / 256, radius=f["radius"], **case["kw"])
        kw.update(flat=res, flat_map=case["flat"]["map"], h_lo=s["h_lo_q"] * size / 256, h_hi=s["h_hi_q"] * size / 256)
    else:
        open_band = s["h_lo_q"] == -cluster.OPEN
        kw.update(z_ref=lo_z + s["z_ref_q"] * size / 256, h_lo=None if open_band else s["h_lo_q"] * size / 256, h_hi=None if open_band else s["h_hi_q"] * size / 256)
    return m.clusters(**dict(kw, **more))


def test_cpu_objects_agree(sv, all_cases, defined):
    """VoxelMap(device="cpu").clusters and .despeckle run the numpy form."""
    rigmod = util.pkg("rig")
    for name in ("sizes_keep", "band", "floor_over_the_floor", "tombstone_carved", "capacity"):
        m = _objects(rigmod, all_cases[name], "cpu", lambda a: a)
        got = {k: v.numpy() for k, v in _object_clusters(rigmod, all_cases[name], m).items()}
        assert _differ(got, defined[name]) == [], name
    c = all_cases["floor_over_the_floor"]
    m = _objects(rigmod, c, "cpu", lambda a: a)
    om = rigmod.OccupancyMap(*cluster.FLOOR_FLAT, device="cpu")
    with pytest.raises(ValueError):
        m.clusters(flat=om)  # not loaded yet
    om.load_voxels(m, step=0.5, height=8.0)
    got = {k: v.numpy() for k, v in m.clusters(flat=om, h_lo=0.5, h_hi=8.0).items()}
    assert _differ(got, defined["floor_over_the_floor"]) == []
    m = _objects(rigmod, all_cases["sizes_keep"], "cpu", lambda a: a)
    claimed = m.stats()["claimed"]
    info = m.despeckle(cluster.SIZES_K)
    assert info.tolist() == defined["sizes_drop"]["info"].tolist() and m.stats()["claimed"] == claimed == 12 and m.rows()["count"] == 9
    assert m.despeckle(cluster.SIZES_K, prune=True).tolist() == [9, 2, 2, 0, 0, 5, 0, 0] and m.stats()["claimed"] == 9
    with pytest.raises(TypeError):
        m.despeckle(3, reach=1)
    with pytest.raises(ValueError):
        m.clusters(flat=3)


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = {"sv_voxel_clusters_device", "sv_voxel_clusters_workspace_bytes", "sv_debug_voxel_clusters"}
    assert set(re.findall(r"\(?\b(sv_\w*voxel_cluster\w*)\)?\s*\(", src)) == names
    assert text.index("/* ---- (V)") < text.index("/* ---- (W)") < text.index("/* ---- (A)") and " *  (W) " in text
    engine = util.pkg("engine")
    assert set(engine.STAGE_SIGNATURES["voxel_clusters"]) == names and set(engine._GROUP_NEEDS["voxel_clusters"]) == {"voxel_map", "occupancy_map"}
    fields = re.search(r"typedef struct \{([^}]*)\} sv_voxel_cluster_spec;", src).group(1)
    declared = [n.strip().split("[")[0] for part in fields.split(";") if part.strip() for n in part.strip().split(" ", 1)[1].split(",")]
    assert declared == [n for n, _ in engine.SvVoxelClusterSpec._fields_] and ctypes.sizeof(engine.SvVoxelClusterSpec) == 64
    assert declared[:8] == list(sv.VOXEL_CLUSTER_WORDS) and len(sv.VOXEL_CLUSTER_INFO) == 6
    build = util.pkg("build")
    assert "voxel_cluster_kernels.hip" in build.SOURCES and "voxel_cluster.cpp" in build.SOURCES and "voxel_cluster_kernels.h" in build.HEADERS
    assert "voxel_map_clusters" in sv.__doc__ and "(W)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_cluster_kernels.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert '#include "voxel_map_table.h"' in source and '#include "wave_ops.h"' in source and "asm" not in code and "float" not in code
    # the table's and the flat map's own rules: none restated; every link goes through the table's probe
    assert code.count("vmap_passes(") == 1 and code.count("vmap_centre(") == 2 and code.count("map_cell(") == 1 and code.count("map_grid(") == 2
    assert code.count("vmap_find(") == 1 and code.count("vmap_slot_of(") == 1 and code.count("vmap_clear_values(") == 1 and "0x9E3779B97F4A7C15" not in code and "0xFFFFF" not in code
    # no grid barrier, no cooperative launch, no flag to wait for; in the link kernel parent[] goes through the agent-scope atomics only
    assert "cooperative" not in code.lower() and "grid.sync" not in code and "__threadfence" not in code and "while (!" not in code
    link = code[code.index("void k_vcluster_link"):code.index("void k_vcluster_roots")]
    assert "a.parent[" not in link and "agent_load(a.parent" in link and "agent_unite(a.parent" in link and "__syncthreads" not in link and "__shfl" not in link
    for name in ("agent_load", "agent_find", "agent_unite"):
        body = code[code.index(" %s(" % name):]
        assert "__HIP_MEMORY_SCOPE_AGENT" in body[:body.index("\n}")] or name == "agent_find", name
    assert "Termination." in source and "ONLY LAUNCH IN WHICH A WORKGROUP READS" in source
    host = open(os.path.join(build.CSRC, "voxel_cluster.cpp")).read()
    assert "check_voxel_map(" in host and "check_map(" in host and "map_cells_of(" in host and "outputs_overlap(" in host and "hipMalloc" not in host + source
    assert "Synchronize" not in host + source
    assert "VCLUSTER_CAPACITY_MAX = 65535" in open(os.path.join(build.CSRC, "voxel_cluster_kernels.h")).read() and sv.VOXEL_CLUSTER_CAPACITY_MAX == 65535


def _aligned(words, fill, offset_words=0):
    """A host int64 array of `words` words that starts 16-byte aligned plus offset_words words."""
    raw = np.full(words + 3, fill, np.int64)
    skip = ((-raw.ctypes.data) % 16) // 8 + offset_words
    return raw, raw[skip:skip + words]


def test_the_c_entry_refuses(sv, eng):
    """Every check of the C entry runs before any HIP call: host memory stands in for the device buffers, and stays as it was."""
    L = eng.voxel_clusters_lib()
    spec = eng.voxel_map_spec(sv.voxel_map_params(**BOX16))
    need = L.sv_voxel_map_bytes(512)
    capacity, rows, cols = 4, 3, 4
    ws = L.sv_voxel_clusters_workspace_bytes(512, capacity)
    assert ws == 4 * (2 * 1024 + 2) and L.sv_voxel_clusters_workspace_bytes(512, 0) == 0 and L.sv_voxel_clusters_workspace_bytes(512, 65536) == 0
    assert L.sv_voxel_clusters_workspace_bytes(0, 4) == 0 and L.sv_voxel_clusters_workspace_bytes(2 ** 26 + 1, 4) == 0
    assert L.sv_voxel_clusters_workspace_bytes(2 ** 26, 65535) == 4 * (2 * 2 ** 27 + 2 * 2 ** 17)
    held = {k: _aligned(words, 7)[1] for k, words in (("map", need // 8), ("floor", rows * cols // 2), ("label", 512), ("clusters", 16 * capacity), ("info", 8), ("workspace", ws // 8 + 1))}
    outputs = ("label", "clusters", "info", "workspace")
    good = dict({k: v.ctypes.data for k, v in held.items()}, map_bytes=need, spec=spec, cluster=eng.voxel_cluster_spec(cluster.words(mode=1, capacity=capacity)),
                flat=eng._occupancy_map_struct(cluster.flat_words((0, rows), (0, cols), 1)), min_n=1, min_rows=1, since=0, workspace_bytes=ws)

    def call(**change):
        a = dict(good, **change)
        ref = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731
        return L.sv_voxel_clusters_device(a["map"], a["map_bytes"], ref(a["spec"]), ref(a["cluster"]), ref(a["flat"]), a["floor"], a["min_n"], a["min_rows"], a["since"],
                                          a["label"], a["clusters"], a["info"], a["workspace"], a["workspace_bytes"], None)

    def flat_with(**words):
        return eng._occupancy_map_struct(dict(cluster.flat_words((0, rows), (0, cols), 1), **words))

    def cluster_with(**words):
        s = eng.voxel_cluster_spec(cluster.words(mode=1, capacity=capacity))
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
    bad += [(dict(cluster=None), b"cluster is NULL")] + [(dict(cluster=cluster_with(reserved=k)), b"reserved") for k in (0, 7)]
    bad += [(dict(cluster=cluster_with(**w)), text) for w, text in ((dict(connectivity=8), b"connectivity"), (dict(connectivity=0), b"connectivity"), (dict(mode=2), b"mode"),
                                                                   (dict(mode=-1), b"mode"), (dict(mode=0, z_ref_q=(1 << 30) + 1), b"z_ref_q"),
                                                                   (dict(mode=0, z_ref_q=-(1 << 30) - 1), b"z_ref_q"), (dict(h_lo_q=-(1 << 30) - 1), b"band"),
                                                                   (dict(h_hi_q=(1 << 30) + 1), b"band"), (dict(h_lo_q=7, h_hi_q=7), b"band"), (dict(min_voxels=0), b"min_voxels"),
                                                                   (dict(capacity=0), b"capacity"), (dict(capacity=65536), b"capacity"), (dict(drop=2), b"drop"), (dict(drop=-1), b"drop"))]
    bad += [(dict(flat=None), b"map spec"), (dict(flat=flat_with(rows=0)), b"rows"), (dict(flat=flat_with(scale=0)), b"scale"), (dict(flat=flat_with(top=1 << 24)), b"top"),
            (dict(floor=None), b"floor is NULL"), (dict(floor=good["floor"] + 2), b"floor is not 4-byte")]
    bad += [(dict(min_n=0), b"min_n"), (dict(min_n=-5), b"min_n")]
    bad += [(dict(**{k: None}), k.encode()) for k in outputs]
    bad += [(dict(clusters=good["clusters"] + 4), b"8-byte"), (dict(info=good["info"] + 4), b"8-byte"), (dict(label=good["label"] + 2), b"4-byte"), (dict(workspace=good["workspace"] + 2), b"4-byte")]
    bad += [(dict(workspace_bytes=ws - 1), b"workspace_bytes"), (dict(workspace_bytes=0), b"workspace_bytes")]
    bad += [(dict(**{k: good["map"] + 64}), b"shares") for k in outputs] + [(dict(**{k: good["floor"]}), b"shares") for k in outputs]
    bad += [(dict(**{b: good[a] + 8}), b"shares") for i, a in enumerate(outputs) for b in outputs[i + 1:]]
    bad += [(dict(info=good["label"] + 4 * 1024 - 8), b"shares"), (dict(info=good["clusters"] - 56), b"shares")]  # the last and the first byte
    for change, text in bad:
        eng.lib().sv_last_error(None)
        assert call(**change) == SV_ERR_ARG, change
        said = eng.lib().sv_last_error(None)
        assert said and said.startswith(b"sv_voxel_clusters") and text in said, (change, said)
    assert all((v == 7).all() for v in held.values())
    assert eng.debug_voxel_clusters(0, 0) == 0 and eng.debug_voxel_clusters(2049, 8) == 0 and eng.debug_voxel_clusters(-1, -1) == 0 and eng.debug_voxel_clusters(0, 64) == 0
    assert eng.debug_voxel_clusters(7, 0) == 0 and eng.debug_voxel_clusters(0, 0) == 7


# ---------------------------------------------------------------------------------------------------------------- GPU

def _host(eng, res):
    key, label = eng.voxel_cluster_labels(res)
    return dict(clusters=res.clusters.cpu().numpy(), info=res.info.cpu().numpy(), key=key.cpu().numpy(), label=label.cpu().numpy())


@pytest.fixture(scope="module")
def device_maps(sv, eng, all_cases):
    """Per case a VoxelMap on the device after the case's ops, built once; the tests that change one build their own."""
    rigmod = util.pkg("rig")
    return {name: _objects(rigmod, c, "cuda", _cuda) for name, c in all_cases.items()}


@pytest.mark.gpu
def test_the_device_against_the_numpy_form(sv, eng, all_cases, defined, device_maps):
    """Every case; then every case again with the table walked by one workgroup, whose lanes make four trips over 1024 slots."""
    rigmod = util.pkg("rig")
    for groups in (0, 1):
        eng.debug_voxel_clusters(groups)
        try:
            for name, case in all_cases.items():
                m = _objects(rigmod, case, "cuda", _cuda) if case["spec"]["drop"] else device_maps[name]
                before = m.buffer.clone()
                got = _host(eng, _object_clusters(rigmod, case, m))
                assert _differ(got, defined[name]) == [], (groups, name, got["info"].tolist(), defined[name]["info"].tolist())
                assert case["spec"]["drop"] or bool((m.buffer == before).all()), name  # the voxel map is only read
        finally:
            assert eng.debug_voxel_clusters(0) == groups


@pytest.mark.gpu
def test_the_kernels_choices_change_no_bit(sv, eng, all_cases, defined, device_maps):
    """One atomic per member instead of the wavefront's combine, and the link kernel without path compression: the same result."""
    rigmod = util.pkg("rig")
    try:
        for flags in (16, 32, 48):
            eng.debug_voxel_clusters(0, flags)
            for name in ("slab", "snake_forward", "schedule_in_order", "floor_over_the_floor", "capacity", "probe"):
                got = _host(eng, _object_clusters(rigmod, all_cases[name], device_maps[name]))
                assert _differ(got, defined[name]) == [], (flags, name)
    finally:
        eng.debug_voxel_clusters(0, 0)


@pytest.mark.gpu
def test_the_schedule_moves_the_slots_not_the_result(sv, eng, all_cases, defined, device_maps):
    layouts = [device_maps["schedule_" + k].clusters().keys.cpu().numpy() for k in ("in_order", "reversed", "shuffled")]
    assert all(sorted(a[a != -1].tolist()) == sorted(layouts[0][layouts[0] != -1].tolist()) for a in layouts)
    assert any(a.tobytes() != layouts[0].tobytes() for a in layouts[1:])  # where an entry lies follows the inserts
    probe = device_maps["probe"].clusters().keys.cpu().numpy()
    held = [int(k) for k in probe[[1022, 1023, 0, 1]] if k != -1]
    assert len(held) >= 3 and all(int(sv.voxel_map_slot_of(k, 1024)) == cluster.PROBE_SLOT for k in held[:3])  # a chain around the table's end


@pytest.mark.gpu
def test_twice_into_the_same_outputs(sv, eng, all_cases, defined, device_maps):
    """The clear is complete: outputs and workspace full of other numbers - an earlier case's, then all ones - come out the same."""
    m, case = device_maps["schedule_in_order"], all_cases["schedule_in_order"]
    words = m.params
    res = eng.voxel_map_clusters(m.buffer, words, spec=case["spec"])
    assert _differ(_host(eng, res), defined["schedule_in_order"]) == []
    for fill in (None, -1, 0x7F7F7F7F):
        if fill is not None:
            for k in ("rows", "info", "label", "workspace"):
                getattr(res, k).fill_(fill)
        again = eng.voxel_map_clusters(m.buffer, words, spec=case["spec"], out=res)
        assert again.rows.data_ptr() == res.rows.data_ptr() and again.workspace.data_ptr() == res.workspace.data_ptr(), fill
        assert _differ(_host(eng, again), defined["schedule_in_order"]) == [], fill
    other = eng.voxel_map_clusters(device_maps["slab"].buffer, words, spec=all_cases["slab"]["spec"], out=res)  # the same box and capacity
    assert _differ(_host(eng, other), defined["slab"]) == []
    lost = device_maps["overflowed"]
    assert _differ(_host(eng, eng.voxel_map_clusters(lost.buffer, lost.params, spec=all_cases["overflowed"]["spec"])), defined["overflowed"]) == []
    for kw in (dict(out=res.rows), dict(min_n=0), dict(since=2 ** 31), dict(connectivity=7), dict(capacity=0), dict(mode=1), dict(h_lo=1.0, h_hi=0.5)):
        with pytest.raises(ValueError):
            eng.voxel_map_clusters(m.buffer, words, **kw)


@pytest.mark.gpu
def test_stops_after_a_given_kernel(sv, eng, all_cases, defined, device_maps):
    """sv_debug_voxel_clusters' second word: after init nothing is counted; after count the info stands and no row is written; after
    rank the rows hold their voxels and nothing else."""
    m, case, want = device_maps["schedule_in_order"], all_cases["schedule_in_order"], defined["schedule_in_order"]
    run = lambda: eng.voxel_map_clusters(m.buffer, m.params, spec=case["spec"], sort=False)  # noqa: E731
    try:
        eng.debug_voxel_clusters(0, 1)
        got = run()
        assert not got.info.cpu().numpy().any() and not got.clusters.cpu().numpy().any()
        eng.debug_voxel_clusters(0, 4)
        got = run()
        assert got.info.cpu().numpy().tolist() == want["info"].tolist() and not got.clusters.cpu().numpy().any()
        eng.debug_voxel_clusters(0, 6)
        rows = run().clusters.cpu().numpy()
        assert sorted(rows[:15, 1].tolist()) == sorted(want["clusters"][:, 1].tolist()) and not rows[15:].any() and not rows[:, 2].any()
    finally:
        eng.debug_voxel_clusters(0, 0)
    assert _differ(_host(eng, eng.voxel_map_clusters(m.buffer, m.params, spec=case["spec"])), want) == []


@pytest.mark.gpu
def test_cut_rows_before_and_behind_the_sort(sv, eng, all_cases, defined, device_maps):
    """70 kept components at 64 rows: the C entry's own rows are some 64 of the 70; sorted, they are the 64 least keys."""
    m, case = device_maps["capacity"], all_cases["capacity"]
    raw = eng.voxel_map_clusters(m.buffer, m.params, spec=case["spec"], sort=False)
    rows, info, label = raw.clusters.cpu().numpy(), raw.info.cpu().numpy(), raw.label.cpu().numpy()
    keys = defined["capacity"]["key"]
    assert rows.shape == (64, 16) and info[:3].tolist() == [70, 70, 70] and len(set(rows[:, 0].tolist())) == 64 and set(rows[:, 0].tolist()) <= set(keys.tolist())
    assert (label == -3).sum() == 6 and sorted(label[label >= 0].tolist()) == list(range(64)) and (label == -1).sum() == 1024 - 70
    table = raw.keys.cpu().numpy()
    assert all(rows[label[s], 0] == table[s] for s in np.flatnonzero(label >= 0))  # single voxels: a row's least key is its voxel's
    got = _host(eng, eng.voxel_map_clusters(m.buffer, m.params, spec=case["spec"]))
    assert _differ(got, defined["capacity"]) == [] and got["clusters"][:, 0].tolist() == keys[:64].tolist()


@pytest.mark.gpu
def test_a_drop_and_what_follows_it(sv, eng, all_cases, defined):
    """despeckle() on the device and in numpy: rows(), flatten() and a second clusters() skip what was emptied, claimed stays, and
    prune() frees the slots."""
    rigmod = util.pkg("rig")
    flat = cluster.flat_words((0, 16), (0, 16), 1)
    got = {}
    for device, to in (("cuda", _cuda), ("cpu", lambda a: a)):
        m = _objects(rigmod, all_cases["sizes_keep"], device, to)
        steps = dict(info=m.despeckle(cluster.SIZES_K).cpu().numpy(), claimed=np.array(m.stats()["claimed"]), count=np.array(m.rows()["count"]), key=m.rows()["key"].cpu().numpy())
        steps["drawn"] = m.flatten(flat, z_ref=0.0).stats.cpu().numpy()
        again = m.clusters(min_voxels=1)
        steps.update({"again_" + k: v for k, v in (_host(eng, again) if device == "cuda" else {k: v.numpy() for k, v in again.items()}).items()})
        pruned = m.prune()
        steps["pruned"] = np.asarray(pruned.cpu().numpy() if device == "cuda" else [pruned[k] for k in sv.VOXEL_CARRY_STATS])
        steps["claimed_after"] = np.array(m.stats()["claimed"])
        got[device] = steps
    cpu = got["cpu"]
    assert cpu["info"].tolist() == defined["sizes_drop"]["info"].tolist() and cpu["info"][EMPTIED] == cpu["info"][SMALL] == 3
    assert cpu["claimed"] == 12 and cpu["count"] == 9 and cpu["drawn"][0] == 9 and cpu["again_info"][:3].tolist() == [9, 2, 2] and cpu["again_label"].tolist() == [-1] * 3 + [0] * 4 + [1] * 5
    assert cpu["pruned"][:2].tolist() == [9, 3] and cpu["claimed_after"] == 9
    assert [k for k in cpu if not (got["cuda"][k].shape == cpu[k].shape and got["cuda"][k].dtype == cpu[k].dtype and got["cuda"][k].tobytes() == cpu[k].tobytes())] == []


@pytest.mark.gpu
def test_end_to_end_on_the_device(sv, eng, all_cases, defined):
    """update -> flatten (load_voxels) -> clusters(floor) -> boxes: the posts and the wall that stand on the ground, in metres."""
    rigmod = util.pkg("rig")
    c = all_cases["floor_over_the_floor"]
    m = _objects(rigmod, c, "cuda", _cuda)
    om = rigmod.OccupancyMap(*cluster.FLOOR_FLAT, device="cuda")
    loaded = om.load_voxels(m, step=0.5, height=8.0)
    found = m.clusters(flat=om, h_lo=0.5, h_hi=8.0)
    assert _differ(_host(eng, found), defined["floor_over_the_floor"]) == []
    assert int(found.info[MEMBERS]) == int(loaded.stats[4])  # (V)'s obstacle voxels
    boxes = eng.voxel_cluster_boxes(found, m.params)
    want = sv.voxel_cluster_boxes(defined["floor_over_the_floor"]["clusters"], m.params)
    assert all(boxes[k].dtype == want[k].dtype and boxes[k].tobytes() == want[k].tobytes() for k in want)
    posts = sorted([x + 0.5, y + 0.5, 2.5] for x, y in cluster.FLOOR_POSTS)
    assert sorted(boxes["centre"].tolist()) == sorted(posts + [[8.0, 12.5, 2.0]])
    wall = boxes["voxels"].tolist().index(8)
    assert boxes["lo"][wall].tolist() == [6.0, 12.0, 1.0] and boxes["hi"][wall].tolist() == [10.0, 13.0, 3.0]
    whole = m.clusters()
    assert whole.info.cpu().tolist()[:3] == [272, 1, 1] and whole.label.data_ptr() != 0


@pytest.mark.gpu
def test_cli_voxel_clusters(sv, eng, tmp_path, capsys):
    """--voxel-clusters writes <FILE>.clusters.txt and .clusters.ply at the end of the run, over the flat map's floor with --voxel-flatten."""
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
    for bad in (full + ["--voxel-clusters", "5"], full + ["--voxel-map", str(tmp_path / "no.ply"), "--voxel-clusters", "5,7"],
                full + ["--voxel-map", str(tmp_path / "no.ply"), "--voxel-clusters", "0"]):
        with pytest.raises(SystemExit):
            sv.main(bad)
    assert not os.path.exists(tmp_path / "no.ply")
    capsys.readouterr()
    for extra, stem in (([], "free"), (["--voxel-flatten=-5,45,-20,20,2,0.3"], "floor")):
        sv.main(full + ["--voxel-map", str(tmp_path / (stem + ".ply")), "--voxel-clusters", "5,18"] + extra)
        said = [line for line in capsys.readouterr().out.splitlines() if line.startswith("voxel map clustered: ")]
        assert len(said) == 1
        members, components, kept, _, largest = (int(w) for w in re.findall(r"\d+", said[0].split(", written")[0]))
        lines = [line.split() for line in open(tmp_path / (stem + ".clusters.txt")).read().splitlines()]
        assert len(lines) == kept > 0 and components >= kept and all(len(line) == 13 for line in lines)
        voxels = [int(line[1]) for line in lines]
        assert min(voxels) >= 5 and max(voxels) == largest and [int(line[0]) for line in lines] == sorted(int(line[0]) for line in lines)
        assert all(float(line[5 + k]) < float(line[2 + k]) < float(line[8 + k]) for line in lines for k in range(3))  # the centre inside the box
        assert all(0 <= int(line[11]) <= int(line[12]) <= n - 1 for line in lines)
        head = open(tmp_path / (stem + ".clusters.ply"), "rb").read(200).decode("latin1")
        assert "element vertex %d\n" % sum(voxels) in head and sum(voxels) <= members
