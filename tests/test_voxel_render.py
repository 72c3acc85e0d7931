"""The voxel map rendered into a camera (group (U)): stereo_vision.sv.voxel_map_render against hand numbers and its plain-loop form, and
engine.voxel_map_render / rig.VoxelMap.render / the CLI against the definition.  Every comparison is shape, dtype and bytes."""
import ctypes
import os
import re

import numpy as np
import pytest

import util
import voxel_render_cases as render
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from voxel_map_cases import BOX16, IDENTITY, cell_points, one_frame

SV_ERR_ARG = -1
IMAGES = ("depth", "key", "color", "disparity", "stats", "label", "counts")


def _same_arrays(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes())


def _differ(got, want, fields=IMAGES):
    return [k for k in fields if not _same_arrays(got[k], want[k])]


def _define(sv, case):
    state, seq = sv.voxel_map_state(sv.voxel_map_params(**case["params"])), 0
    for call in case["calls"]:
        sv.voxel_map_insert(state, *call, seq0=seq)
        seq += call[0].shape[0]
    return state


@pytest.fixture(scope="module")
def all_cases(sv):
    return render.all_cases(sv)


@pytest.fixture(scope="module")
def defined(sv, all_cases):
    """Per case the numpy form's render, computed once and left as it is."""
    return {name: sv.voxel_map_render(_define(sv, c), c["cams"], c["camera"], c["measured"], **c["kw"]) for name, c in all_cases.items()}


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_hand_case(sv):
    """Identity camera, f = 8, no square (half_px = 0).  A = (1.5, 1.5, 2.5) + 1 / 131072 per axis and B = (3, 3, 5) + 1 / 131072 lie on one
    ray, u = v = 4.8: pixel (5, 5), where A wins with zq = int(2.5000076 * 256) = 640.  C = (0.5, 0.5, 4.5) + 1 / 131072 is alone at u = v
    = 0.89: pixel (1, 1), zq = int(4.5000076 * 256) = 1152.  q32 = 2, q33 = 0: e = 8 / ((zq + 0.5) / 256) / 2."""
    case = render.hand_case()
    got = sv.voxel_map_render(_define(sv, case), case["cams"], case["camera"])
    depth, key, color = np.full((1, 7, 8), -1, np.int32), np.full((1, 7, 8), -1, np.int64), np.zeros((1, 7, 8, 4), np.uint8)
    disparity = np.full((1, 7, 8), -1, np.float32)
    depth[0, 5, 5], key[0, 5, 5], color[0, 5, 5], disparity[0, 5, 5] = 640, 1 | 1 << 20 | 2 << 40, (10, 20, 30, 40), np.float32(8.0 / (640.5 / 256.0) / 2.0)
    depth[0, 1, 1], key[0, 1, 1], color[0, 1, 1], disparity[0, 1, 1] = 1152, 4 << 40, (90, 100, 110, 120), np.float32(8.0 / (1152.5 / 256.0) / 2.0)
    want = dict(depth=depth, key=key, color=color, disparity=disparity, stats=np.array([[3, 2]], np.int64), label=None, counts=None)
    assert _differ(got, want) == []
    assert abs(float(disparity[0, 5, 5]) - 1.59875) < 1e-5  # the rig would measure 8 / 2.502 / 2 pixels there
    # without the nearer voxel the farther one shows: zq = int(5.0000076 * 256) = 1280
    far = sv.voxel_map_render(_define(sv, case), case["cams"], case["camera"], near=3.0)
    assert far["depth"][0, 5, 5] == 1280 and far["key"][0, 5, 5] == 3 | 3 << 20 | 5 << 40 and far["stats"].tolist() == [[2, 2]]


def test_vectorised_against_brute(sv, all_cases, defined):
    for name, c in all_cases.items():
        brute = sv.voxel_map_render_brute(_define(sv, c), c["cams"], c["camera"], c["measured"], **c["kw"])
        assert _differ(defined[name], brute) == [], name


def test_the_cases_show_what_they_are_for(sv, all_cases, defined):
    d = defined
    assert d["depth_order"]["stats"].tolist() == [[4, 2]]
    for name in ("equal_depth_ab", "equal_depth_ba"):  # two squares of 9 x 9 pixels and one zq
        keys = {render.key_of(np.floor(call[0][0, 0]).astype(np.int64)) for call in all_cases[name]["calls"]}
        assert d[name]["stats"][0, 0] == 2 and len(np.unique(d[name]["depth"][d[name]["depth"] >= 0])) == 1
        assert len(keys) == 2 and (d[name]["key"] == min(keys)).sum() == 72 and (d[name]["key"] == max(keys)).sum() == 9  # 8 rows of either lie in the image: the overlap goes to the smaller
    assert _differ(d["equal_depth_ab"], d["equal_depth_ba"]) == []
    covered = {k: d["footprint_" + k]["stats"][0, 1] for k in ("r0", "r_at_r_max", "r_capped", "r_below_integer", "r_at_integer", "r_largest")}
    assert covered == {"r0": 1, "r_at_r_max": 25, "r_capped": 25, "r_below_integer": 9, "r_at_integer": 25, "r_largest": 9 * 16}
    assert d["footprint_borders"]["stats"].tolist() == [[1, 15]] * 4 + [[1, 9]] * 2 + [[1, 5], [1, 1]] + [[0, 0]] * 4
    assert d["depth_near_kept"]["stats"].tolist() == [[2, 2]] + [[0, 0]] * 4 and d["depth_far_dropped"]["stats"].tolist() == [[0, 0]] * 5
    assert [d["filter_" + k]["stats"][0, 0] for k in ("none", "min_n", "min_rows", "since")] == [4, 3, 3, 3]
    assert len({d["filter_" + k]["key"].tobytes() for k in ("none", "min_n", "min_rows", "since")}) == 4  # each drops another voxel
    assert d["table_wrap"]["stats"][:, 0].min() >= 1
    counts = d["comparison"]["counts"]
    assert (counts > 0).all() and (counts.sum(1) == 9 * 40).all()
    assert d["overflowed"]["stats"].tolist() == [[-1, 0]] * 2 and (d["overflowed"]["depth"] == -1).all() and set(np.unique(d["overflowed"]["label"])) == {0, 1}
    assert d["empty"]["stats"].tolist() == [[0, 0]] * 2 and (d["empty"]["key"] == -1).all() and not d["empty"]["color"].any() and (d["empty"]["disparity"] == -1).all()
    assert d["views_0"]["depth"].shape == (0, 5, 70) and d["views_9_one_pixel"]["stats"][:, 1].tolist() == [1] * 9


def test_comparison_labels(sv, all_cases, defined):
    """Without `measured` there is neither label nor counts and the rest is the same; one float above the pixel at tol is no longer agreed."""
    c, want = all_cases["comparison"], defined["comparison"]
    state = _define(sv, c)
    plain = sv.voxel_map_render(state, c["cams"], c["camera"])
    assert plain["label"] is None and plain["counts"] is None and _differ(plain, want, IMAGES[:5]) == []
    z = ((want["depth"].astype(np.float64) + 0.5) / 256.0) * 1.0
    e = (c["camera"]["f"] / z - c["camera"]["q33"]) / c["camera"]["q32"]
    at = tuple(np.argwhere((want["depth"] >= 0) & (c["measured"].astype(np.float64) - e == c["kw"]["tol"]))[0])
    assert want["label"][at] == 3
    more = c["measured"].copy()
    more[at] = np.nextafter(more[at], np.float32(np.inf))
    assert sv.voxel_map_render(state, c["cams"], c["camera"], more, **c["kw"])["label"][at] == 4


def test_helpers(sv):
    # voxel_render_cams undoes voxel_map_pose and the rig's transform: the camera point p lies in the world at R (XR p + XT) + t
    rng = np.random.default_rng(3)
    poses = sv.voxel_map_pose(rng.uniform(-50, 50, 6), rng.uniform(-50, 50, 6), rng.uniform(-3, 3, 6), rng.uniform(-1, 1, 6))
    XT = np.array([0.3, -0.1, 1.6])
    cams = sv.voxel_render_cams(poses, sv.CAMERA_TO_VEHICLE, XT)
    assert cams.shape == (6, 12) and cams.dtype == np.float64
    for pose, cam in zip(poses, cams):
        R, t, Rc, tc = pose[:9].reshape(3, 3), pose[9:], cam[:9].reshape(3, 3), cam[9:]
        assert np.abs(Rc @ (R @ XT + t) + tc).max() < 1e-12  # the camera's centre, which is XT in the vehicle's axes
        assert np.abs(Rc @ t + tc - sv.CAMERA_TO_VEHICLE.T @ (0 - XT)).max() < 1e-12  # the vehicle's origin, seen from the camera
        p = rng.uniform(-5, 5, 3)
        assert np.abs(Rc @ (R @ (sv.CAMERA_TO_VEHICLE @ p + XT) + t) + tc - p).max() < 1e-12
    assert np.array_equal(sv.voxel_render_cams(IDENTITY[None]), IDENTITY[None])
    assert sv.voxel_render_cams(np.array([[1.0, 2.0, 1.0, 0.0]])).tolist() == [[1, 0, 0, 0, 1, 0, 0, 0, 1, -1, -2, 0]]
    Q = np.array([[1, 0, 0, -609.5], [0, 1, 0, -172.8], [0, 0, 0, 721.5], [0, 0, 1.86, 0.01]])
    cam = sv.voxel_render_camera(Q, 1242, 375, 0.2)
    assert cam == dict(f=721.5, cx=609.5, cy=172.8, q32=1.86, q33=0.01, width=1242, height=375, size=0.2, half_px=0.5 * 721.5)
    assert sv.voxel_render_camera(Q, 1242, 375, 0.2, footprint=2.0)["half_px"] == 721.5
    for at, value in (((0, 0), 2.0), ((0, 1), 0.1), ((1, 2), 0.1), ((2, 2), 1.0), ((3, 0), 0.5), ((2, 3), 0.0), ((2, 3), -1.0), ((3, 2), 0.0), ((3, 3), np.nan), ((0, 3), np.inf)):
        bad = Q.copy()
        bad[at] = value
        with pytest.raises(ValueError):
            sv.voxel_render_camera(bad, 1242, 375, 0.2)
    for kw in (dict(width=0), dict(height=8193), dict(size=0.0), dict(size=np.nan), dict(footprint=-1.0)):
        with pytest.raises(ValueError):
            sv.voxel_render_camera(Q, **dict(dict(width=1242, height=375, size=0.2), **kw))
    state = sv.voxel_map_state(sv.voxel_map_params(**BOX16))
    for kw in (dict(min_n=0), dict(r_max=9), dict(r_max=-1), dict(near=0.0), dict(near=2.0, far=2.0), dict(far=2.0 ** 20 + 1), dict(near=np.nan),
               dict(measured=np.zeros((1, 9, 16), np.float32), tol=-1.0), dict(measured=np.zeros((1, 9, 16), np.float32), tol=np.nan), dict(measured=np.zeros((1, 9, 15), np.float32)),
               dict(measured=np.zeros((1, 9, 16), np.float64))):
        with pytest.raises(ValueError):
            sv.voxel_map_render(state, IDENTITY[None], render.camera(), **kw)
    with pytest.raises(ValueError):
        sv.voxel_map_render(state, IDENTITY[None, :11], render.camera())
    with pytest.raises(ValueError):
        sv.voxel_map_render(state, IDENTITY[None], dict(render.camera(), f=0.0))
    assert sv.cli_voxel_render_spec("out") == ("out", 1.0) and sv.cli_voxel_render_spec("a,b,0.5") == ("a,b", 0.5)
    assert sv.cli_voxel_render_text([1, 2, 3, 4, 5, 6]) == "none 1, measured 2, expected 3, agree 4, nearer 5, farther 6"
    for bad in (",1", "out,-1", "out,nan"):
        with pytest.raises(ValueError):
            sv.cli_voxel_render_spec(bad)


def _round_trip(sv):
    """A 64 x 9 D1 of one disparity, through compact_cloud into a map at the identity pose, and the camera that renders it back."""
    f, b, d0, size = 64.0, 0.5, 4.0, 0.5  # Z = f b / d0 = 8 m = 16 cells: f size / Z = 4 pixels per voxel; footprint 2: r = int(3.99..) = 3, and 2 r + 1 pixels span a voxel's 4
    Q = np.array([[1, 0, 0, -32.0], [0, 1, 0, -4.0], [0, 0, 0, f], [0, 0, 1.0 / b, 0.0]])
    d1 = np.full((9, 64), d0, np.float32)
    xyz, _, _ = sv.compact_cloud(d1, Q, dtype="f64")
    params = dict(lo=(-8.0, -2.0, 0.0), hi=(8.0, 2.0, 16.0), size=size, capacity=1024)
    state = sv.voxel_map_state(sv.voxel_map_params(**params))
    sv.voxel_map_insert(state, xyz[None], None, None, np.array([len(xyz)], np.int32), IDENTITY[None])
    return Q, d1, params, xyz, state, sv.voxel_render_camera(Q, 64, 9, size, footprint=2.0)


def _round_trip_bound(Q, size, z):
    """See test_round_trip."""
    return 2.0 * (Q[2, 3] / Q[3, 2]) / z ** 2 * (size / 65536.0 + size / 512.0)


def test_round_trip(sv):
    """Every pixel of a constant D1 = d0 reprojects to Z = f b / d0 and is inserted at the identity pose; the render with the same Q at the
    same pose must give the disparity back.  What lies between: a voxel's centre is the mean of offsets quantised to 1 / 65536 of a cell
    (rounded down, and given back with half a step added: at most size / 65536 off in z), and the rendered depth is the middle of a step
    of zq, 1 / 256 of a cell wide: at most size / 512 off.  With d = f b / z, |dd| = f b / z^2 |dz|, so |e - d0| <= f b / Z^2 *
    (size / 65536 + size / 512); the bound is that, doubled.  Here f b / Z^2 = 0.5 per metre: about 0.001 pixels."""
    Q, d1, params, xyz, state, cam = _round_trip(sv)
    Z = float(xyz[0, 2])
    assert Z == 8.0 and cam["f"] * params["size"] / Z >= 2
    bound = _round_trip_bound(Q, params["size"], Z)
    assert 0.0005 < bound < 0.002
    seen = sv.voxel_map_render(state, IDENTITY[None], cam, d1[None], tol=bound)
    inner = (slice(0, 1), slice(1, 8), slice(1, 63))
    assert (seen["depth"][inner] >= 0).all() and seen["stats"][0, 0] == len(state["key"]) > 30
    covered = seen["depth"] >= 0
    assert np.abs(seen["disparity"][covered].astype(np.float64) - 4.0).max() <= bound
    assert (seen["label"][covered] == 3).all() and seen["counts"][0, 3] == covered.sum()
    painted = d1[None].copy()
    painted[0, 2:5, 10:13], painted[0, 4:7, 40:43] = 6.0, 2.5
    seen = sv.voxel_map_render(state, IDENTITY[None], cam, painted, tol=bound)
    want = np.where(covered, 3, 1).astype(np.uint8)
    want[0, 2:5, 10:13], want[0, 4:7, 40:43] = 4, 5
    assert np.array_equal(seen["label"], want) and seen["counts"][0].tolist() == [0, int((~covered).sum()), 0, int(covered.sum()) - 18, 9, 9]


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = {"sv_voxel_render_device", "sv_debug_voxel_render"}
    assert set(re.findall(r"\(?\b(sv_\w*render\w*)\)?\s*\(", src)) == names
    assert text.index("/* ---- (T)") < text.index("/* ---- (U)") < text.index("/* ---- (A)") and " *  (U) " in text
    engine = util.pkg("engine")
    assert set(engine.STAGE_SIGNATURES["voxel_render"]) == names and engine._GROUP_NEEDS["voxel_render"] == ("voxel_map",)
    for word in ("voxel_map", "view", "carve", "carry", "voxel_match", "map_match", "occupancy", "cost", "clearance", "frontier", "ground_", "stixel_"):
        assert not any(word in n for n in names | {"sv_voxel_render_spec"}), word
    fields = re.search(r"typedef struct \{([^}]*)\} sv_voxel_render_spec;", src).group(1)
    declared = [n.strip().split("[")[0] for part in fields.split(";") if part.strip() for n in part.strip().split(" ", 1)[1].split(",")]
    assert declared == [n for n, _ in engine.SvVoxelRenderSpec._fields_] and ctypes.sizeof(engine.SvVoxelRenderSpec) == 96
    build = util.pkg("build")
    assert "voxel_render_kernels.hip" in build.SOURCES and "voxel_render.cpp" in build.SOURCES and "voxel_render_kernels.h" in build.HEADERS
    assert "voxel_map_render" in sv.__doc__ and "(U)" in sv.__doc__
    source = open(os.path.join(build.CSRC, "voxel_render_kernels.hip")).read()
    code = re.sub(r"//.*", "", source)
    assert '#include "voxel_map_table.h"' in source and "asm" not in code
    # integer atomics only - the two minima and one flush of the counters per workgroup in two kernels -, and the map's own rules
    assert sorted(re.findall(r"\batomic\w*\(", code)) == ["atomicAdd(", "atomicAdd(", "atomicMin(", "atomicMin("]
    assert code.count("vmap_passes(") == 1 and code.count("vmap_find(") == 1 and code.count("vmap_centre(") == 1 and "65536.0" not in code
    readout = open(os.path.join(build.CSRC, "voxel_map_kernels.hip")).read()
    assert readout.count("vmap_centre(") == 1 and "65536.0" not in re.sub(r"//.*", "", readout)  # one copy of the centre, in the header
    assert str(render.VIEWS) in re.search(r"VRENDER_VIEWS = (\d+)", open(os.path.join(build.CSRC, "voxel_render_kernels.h")).read()).group(1)


def _aligned(words, fill, offset_words=0):
    """A host int64 array of `words` words that starts 16-byte aligned plus offset_words words."""
    raw = np.full(words + 3, fill, np.int64)
    skip = ((-raw.ctypes.data) % 16) // 8 + offset_words
    return raw, raw[skip:skip + words]


def test_the_c_entry_refuses(sv, eng):
    """Every check of the C entry runs before any HIP call: host memory stands in for the device buffers, and stays as it was."""
    L = eng.voxel_render_lib()
    spec = eng.voxel_map_spec(sv.voxel_map_params(**BOX16))
    need = L.sv_voxel_map_bytes(512)
    V, H, W = 2, 3, 4
    pixels = V * H * W
    held = {k: _aligned(n, 7)[1] for k, n in (("map", need // 8), ("cams", 12 * V), ("depth", pixels // 2), ("key", pixels), ("color", pixels // 2), ("disparity", pixels // 2),
                                              ("measured", pixels // 2), ("label", pixels // 8), ("stats", 2 * V), ("counts", 6 * V))}
    tol, negative, not_a_number = ctypes.c_double(1.0), ctypes.c_double(-1.0), ctypes.c_double(float("nan"))
    good = dict({k: v.ctypes.data for k, v in held.items()}, map_bytes=need, spec=spec, cam=eng.voxel_render_spec(render.camera(W, H)), views=V, min_n=1, min_rows=1,
                since=0, tol=ctypes.addressof(tol))

    def call(**change):
        a = dict(good, **change)
        return L.sv_voxel_render_device(a["map"], a["map_bytes"], None if a["spec"] is None else ctypes.byref(a["spec"]), None if a["cam"] is None else ctypes.byref(a["cam"]),
                                        a["cams"], a["views"], a["min_n"], a["min_rows"], a["since"], a["depth"], a["key"], a["color"], a["disparity"], a["measured"], a["tol"],
                                        a["label"], a["stats"], a["counts"], None)

    def cam_with(**words):
        c = eng.voxel_render_spec(render.camera(W, H))
        for k, v in words.items():
            if k == "reserved":
                c.reserved[2] = v
            else:
                setattr(c, k, v)
        return c

    def spec_with(**words):
        s = eng.voxel_map_spec(sv.voxel_map_params(**BOX16))
        for k, v in words.items():
            setattr(s, k, v)
        return s

    nan, inf = float("nan"), float("inf")
    bad = [(dict(spec=None), b"spec"), (dict(map=None), b"map"), (dict(map=good["map"] + 8), b"map"), (dict(map_bytes=need - 8), b"map"),
           (dict(spec=spec_with(size=0.0)), b"size"), (dict(spec=spec_with(capacity=0)), b"capacity"), (dict(cam=None), b"cam")]
    bad += [(dict(views=-1), b"views"), (dict(views=4097), b"views"), (dict(views=4096, cam=cam_with(width=8192, height=64)), b"2^31")]
    bad += [(dict(cam=cam_with(**w)), text) for w, text in ((dict(width=0), b"width"), (dict(width=8193), b"width"), (dict(height=0), b"height"), (dict(height=8193), b"height"),
                                                            (dict(reserved=1), b"reserved"), (dict(f=nan), b"finite"), (dict(cx=inf), b"finite"), (dict(cy=-inf), b"finite"),
                                                            (dict(q32=nan), b"finite"), (dict(q33=inf), b"finite"), (dict(half_px=nan), b"finite"), (dict(near=nan), b"finite"),
                                                            (dict(far=inf), b"finite"), (dict(f=0.0), b"f > 0"), (dict(f=-8.0), b"f > 0"), (dict(q32=0.0), b"q32"),
                                                            (dict(half_px=-0.5), b"half_px"), (dict(r_max=-1), b"r_max"), (dict(r_max=9), b"r_max"), (dict(near=0.0), b"near"),
                                                            (dict(near=-1.0), b"near"), (dict(near=4.0, far=4.0), b"far"), (dict(far=2.0 ** 20 + 1), b"far"))]
    bad += [(dict(min_n=0), b"min_n"), (dict(min_n=-5), b"min_n")]
    bad += [(dict(tol=None), b"tol"), (dict(tol=ctypes.addressof(negative)), b"tol"), (dict(tol=ctypes.addressof(not_a_number)), b"tol")]
    bad += [(dict(label=None), b"measured"), (dict(counts=None), b"measured"), (dict(measured=None), b"measured"), (dict(measured=None, label=None), b"measured")]
    bad += [(dict(**{k: None}), k.encode()) for k in ("cams", "depth", "key", "stats")]
    bad += [(dict(**{k: good[k] + 4}), b"8-byte") for k in ("cams", "key", "stats", "counts")]
    bad += [(dict(**{k: good[k] + 2}), b"4-byte") for k in ("depth", "color", "disparity", "measured")]
    outputs = ("depth", "key", "color", "disparity", "label", "stats", "counts")
    bad += [(dict(**{k: good["map"] + 64}), b"shares") for k in outputs] + [(dict(**{k: good["cams"] + 8}), b"shares") for k in outputs]
    bad += [(dict(**{k: good["measured"] + 8}), b"shares") for k in outputs]
    bad += [(dict(**{b: good[a] + 8}), b"shares") for i, a in enumerate(outputs) for b in outputs[i + 1:]]
    bad += [(dict(depth=good["key"] + 8 * pixels - 4), b"shares"), (dict(stats=good["depth"] - 16 * V + 8), b"shares")]  # the last and the first byte
    for change, text in bad:
        eng.lib().sv_last_error(None)
        assert call(**change) == SV_ERR_ARG, change
        said = eng.lib().sv_last_error(None)
        assert said and said.startswith(b"sv_voxel_render") and text in said, (change, said)
    assert all((v == 7).all() for v in held.values())
    # the optional outputs may be left out, and no view is no work: both are taken (and with no view nothing is enqueued, nothing is written)
    assert call(views=0) == 0 and call(views=0, cams=None, depth=None, key=None, stats=None, color=None, disparity=None, measured=None, label=None, counts=None, tol=None) == 0
    assert all((v == 7).all() for v in held.values())


# ---------------------------------------------------------------------------------------------------------------- GPU

def _engine_map(eng, sv, case):
    words = sv.voxel_map_params(**case["params"])
    buf, seq = eng.voxel_map_new(words), 0
    for call in case["calls"]:
        eng.voxel_map_insert(buf, words, *(None if a is None else _cuda(a) for a in call[:4]), call[4], seq0=seq)
        seq += call[0].shape[0]
    return buf, words


def _engine_render(eng, buf, words, case, **more):
    kw = dict(case["kw"], **more)
    measured = kw.pop("measured", case["measured"])
    return eng.voxel_map_render(buf, words, case["cams"], case["camera"], None if measured is None else _cuda(measured), **kw)


def _host(res):
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in IMAGES}


@pytest.mark.gpu
def test_the_device_against_the_numpy_form(sv, eng, all_cases, defined):
    """Every case; then every case again with the table walked by three workgroups, whose last trip is partial in a table of 1024 slots."""
    for groups in (0, 3):
        eng.debug_voxel_render(groups)
        try:
            for name, case in all_cases.items():
                buf, words = _engine_map(eng, sv, case)
                before = buf.clone()
                got = _host(_engine_render(eng, buf, words, case))
                assert _differ(got, defined[name]) == [], (groups, name, got["stats"].tolist(), defined[name]["stats"].tolist())
                assert bool((buf == before).all()), name  # the map is only read
        finally:
            assert eng.debug_voxel_render(0) == groups


@pytest.mark.gpu
def test_equal_depth_whatever_the_slots(sv, eng, all_cases, defined):
    """The same two colliding voxels inserted in either order lie in swapped slots, and render to the same bytes."""
    tables, seen = [], []
    for name in ("equal_depth_ab", "equal_depth_ba"):
        buf, words = _engine_map(eng, sv, all_cases[name])
        table = buf[4:4 + 11 * 1024].view(1024, 11)[:, 0].cpu().numpy()
        tables.append(table[table != -1].tolist())
        seen.append(_host(_engine_render(eng, buf, words, all_cases[name])))
    assert len(tables[0]) == 2 and tables[0] == tables[1][::-1]
    assert _differ(seen[0], seen[1]) == [] and _differ(seen[0], defined["equal_depth_ab"]) == []


@pytest.mark.gpu
def test_optional_outputs_and_reuse_and_twice(sv, eng, all_cases, defined):
    import torch
    case, want = all_cases["comparison"], defined["comparison"]
    buf, words = _engine_map(eng, sv, case)
    full = _engine_render(eng, buf, words, case)
    again = _engine_render(eng, buf, words, case)  # the same call into fresh buffers
    assert _differ(_host(full), want) == [] and _differ(_host(again), want) == [] and again.depth.data_ptr() != full.depth.data_ptr()
    # without color / disparity: the rest is the same
    lean = _engine_render(eng, buf, words, case, color=False, disparity=False)
    assert lean.color is None and lean.disparity is None and _differ(_host(lean), want, ("depth", "key", "stats", "label", "counts")) == []
    # without measured: label and counts of `out` stay as they were, the other outputs are the same
    full.label.fill_(9)
    full.counts.fill_(-3)
    plain = _engine_render(eng, buf, words, case, measured=None, out=full)
    assert plain.label is None and plain.counts is None and plain.depth.data_ptr() == full.depth.data_ptr()
    assert _differ(_host(plain), want, IMAGES[:5]) == [] and bool((full.label == 9).all()) and bool((full.counts == -3).all())
    for kw in (dict(out=eng.VoxelRenderResult(depth=torch.zeros(3, dtype=torch.int32, device="cuda"))), dict(min_n=0), dict(r_max=9), dict(tol=-1.0),
               dict(measured=np.zeros((2, 9, 39), np.float32)), dict(near=0.0)):
        with pytest.raises(ValueError):
            _engine_render(eng, buf, words, case, **kw)
    with pytest.raises(ValueError):
        eng.voxel_map_render(buf, words, case["cams"][:, :11], case["camera"])


@pytest.mark.gpu
def test_tombstones_and_prune(sv, eng):
    """A voxel that a later frame's sight line passes through is carved; the render shows what lies behind it, and the same after prune()."""
    rigmod = util.pkg("rig")
    cam = render.camera(cx=8.2, cy=4.2, half_px=6.0)
    centre = np.array([8.5, 8.5, 0.0])  # of the camera, in the frame's axes, which are the world's: it looks along z at the cells (8, 8, .)
    got = {}
    for device in ("cuda", "cpu"):
        m = rigmod.VoxelMap(BOX16["lo"], BOX16["hi"], 1.0, 512, device=device)
        first, second = one_frame(cell_points([(8, 8, 4), (3, 8, 4)]), [(1, 2, 3, 4), (5, 6, 7, 8)]), one_frame(cell_points([(8, 8, 10)]), [(9, 9, 9, 9)])
        for frame in (first, second):
            m.update(*((None if a is None else _cuda(a)) if device == "cuda" else a for a in frame[:4]), frame[4])
        show = lambda: _host(m.render(IDENTITY[None], cam, transform=(np.eye(3), centre)))  # noqa: E731
        before = show()
        xyz, n, counts = ((None if a is None else _cuda(a)) if device == "cuda" else a for a in (second[0], second[2], second[3]))
        res = m.carve(xyz, n, counts, second[4], origin=(8.5, 8.5, 0.5), reach_m=12.0, margin=0, min_miss=1)
        assert (res.stats.cpu().tolist() if device == "cuda" else [res[k] for k in sv.VOXEL_CARVE_STATS])[3] == 1
        carved = show()
        m.prune()
        got[device] = (before, carved, show())
    for before, carved, pruned in got.values():
        assert before["depth"][0, 4, 8] == int((4.0 + 32768.5 / 65536.0) * 256.0) and carved["depth"][0, 4, 8] == int((10.0 + 32768.5 / 65536.0) * 256.0)
        assert before["stats"][0, 0] == 3 and carved["stats"][0, 0] == 2 and _differ(carved, pruned) == []
    assert all(_differ(a, b) == [] for a, b in zip(got["cuda"], got["cpu"]))


@pytest.mark.gpu
def test_round_trip_on_the_device(sv, eng):
    """test_round_trip's map built and rendered by the rig's own objects, with the painted squares."""
    rigmod = util.pkg("rig")
    Q, d1, params, xyz, state, cam = _round_trip(sv)
    bound = _round_trip_bound(Q, params["size"], 8.0)
    painted = d1[None].copy()
    painted[0, 2:5, 10:13], painted[0, 4:7, 40:43] = 6.0, 2.5
    want = sv.voxel_map_render(state, IDENTITY[None], cam, painted, tol=bound)
    m = rigmod.VoxelMap(params["lo"], params["hi"], params["size"], params["capacity"], device="cuda")
    cloud = eng.compact_cloud_from_disparity(_cuda(d1[None]), Q, dtype="f64")
    m.update(cloud[0], None, None, cloud[3], IDENTITY[None])
    got = _host(m.render(IDENTITY[None], cam, measured=_cuda(painted), tol=bound))
    assert _differ(got, want) == [] and got["counts"][0, 4:].tolist() == [9, 9] and got["counts"][0, 2] == 0


@pytest.mark.gpu
def test_cli_voxel_render(sv, eng, tmp_path, capsys):
    """--voxel-render writes two PNGs per frame; before the first insert the map is empty, so frame 0 and 1 hold labels 0 and 1 only."""
    from PIL import Image
    from test_occupancy_map import H, W, _drive_frames
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
    for bad in (full + ["--voxel-render", str(tmp_path / "no")], full + ["--voxel-map", str(tmp_path / "no.ply"), "--voxel-render", str(tmp_path / "no") + ",-1"]):
        with pytest.raises(SystemExit):
            sv.main(bad)
    assert not os.path.exists(tmp_path / "no")
    capsys.readouterr()
    out = tmp_path / "seen"
    sv.main(full + ["--voxel-map", str(tmp_path / "drive.ply"), "--voxel-render", str(out) + ",1.5"])
    said = [line for line in capsys.readouterr().out.splitlines() if line.startswith("voxel map rendered before frame")]
    assert len(said) == n and sorted(os.listdir(out)) == sorted("%06d.%s.png" % (i, k) for i in range(n) for k in ("expected", "change"))
    palette = sv.VOXEL_RENDER_PNG.tolist()
    for i in range(n):
        change, expected = np.asarray(Image.open(out / ("%06d.change.png" % i))), np.asarray(Image.open(out / ("%06d.expected.png" % i)))
        assert change.shape == expected.shape == (H, W, 3)
        labels = {palette.index(c) for c in np.unique(change.reshape(-1, 3), axis=0).tolist()}
        counts = [int(w.split()[-1]) for w in said[i].split(": ")[1].split(", ")]
        assert sum(counts) == H * W and {k for k in range(6) if counts[k]} == labels
        if i < 2:  # the map is empty before the first batch
            assert labels <= {0, 1} and not expected.any()
        else:
            assert sum(counts[2:]) > 100 and expected.any()
