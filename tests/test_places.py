"""Place recognition (group (AC)): stereo_vision.sv.place_descriptor and place_match against their row-by-row and pair-by-pair forms on
inputs that sit on every rule (place_cases.py), a synthetic town that is recognised from a turned and shifted pose, PlaceIndex on CPU
tensors, and the GPU path - shape, dtype and bits - against the numpy forms."""
import os

import numpy as np
import pytest

import place_cases as pc
import util
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)

# The town of place_cases.town(seed), seen again from place 20 turned by 30 degrees and 0.5 m to the side, among 41 places 12 m apart:
# sad / norm of the right key and of the runner-up, measured with the numpy definition.  The test asks for the right key
# and for a runner-up at least twice as far: the worst seed has 3.4 times.
TOWN_SEEDS = (0, 1, 2, 3)
TOWN_RATIOS = ((0.180, 0.656), (0.122, 0.614), (0.192, 0.691), (0.141, 0.634))
TOWN_MARGIN = 2.0
LOCALIZE_HALF = (1.0, 1.0, np.radians(4.0))  # the window localize is given around a guess in the voxel map's tests: metres, metres, radians


@pytest.fixture(scope="module")
def desc_cases(sv):
    return pc.descriptor_cases(sv)


@pytest.fixture(scope="module")
def desc_wanted(sv, desc_cases):
    """The numpy form's result per case, computed once."""
    return {name: pc.call_descriptor(sv.place_descriptor, case) for name, case in desc_cases.items()}


@pytest.fixture(scope="module")
def match_all():
    return pc.match_cases()


@pytest.fixture(scope="module")
def match_wanted(sv, match_all):
    return {name: pc.call_match(sv.place_match, case, want_pair=True) for name, case in match_all.items()}


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_params(sv):
    p = sv.place_params(30.0)
    assert (p["rings"], p["sectors"], p["unit"], p["z_unit"]) == (20, 60, 30.0 / 1024, 5.0 / 255)
    assert p["ring_edge2"].tolist() == [(1024 * r // 20) ** 2 for r in range(21)] and p["r_min2"] == 0
    assert p["dirs"].dtype == np.int32 and p["dirs"][0].tolist() == [16384, 0] and p["dirs"][15].tolist() == [0, 16384] and p["dirs"][30].tolist() == [-16384, 0]
    assert sv.place_params(30.0, r_min=3.0)["r_min2"] == 102 ** 2
    for bad in (dict(rings=0), dict(rings=65), dict(sectors=4), dict(sectors=62), dict(sectors=132), dict(rings=64, sectors=68), dict(z_lo=5.0), dict(r_min=30.0), dict(r_min=-1.0)):
        with pytest.raises(ValueError):
            sv.place_params(30.0, **bad)
    with pytest.raises(ValueError):
        sv.place_params(float("nan"))


def test_descriptor_numpy_equals_brute(sv, desc_cases, desc_wanted):
    for name, case in desc_cases.items():
        if case["xyz"].shape[0] * case["xyz"].shape[1] > 3000:  # row by row in Python: the first frame's first rows will do
            case = dict(case, xyz=case["xyz"][:1, :800], n=None if case["n"] is None else case["n"][:1, :800], counts=np.minimum(case["counts"][:1], 800),
                        poses=None if case["poses"] is None else case["poses"][:1])
            want = pc.call_descriptor(sv.place_descriptor, case)
        else:
            want = desc_wanted[name]
        assert pc.same(pc.call_descriptor(sv.place_descriptor_brute, case), want, pc.DESC_FIELDS), name


def test_descriptor_by_hand(sv):
    p = sv.place_params(30.0, rings=4, sectors=8)
    # ring edges at q = 0, 256, 512, 768; sector k from 45 k degrees on.  z_unit = 5 / 255: z = 1.0 -> 1 + floor(1.5 * 51) = 77
    rows = [pc.at_cell(p, 100, 0), pc.at_cell(p, 100, 0, 2.0), pc.at_cell(p, 0, 300), pc.at_cell(p, -600, -1), pc.at_cell(p, 0, 0), pc.at_cell(p, 800, 800),
            pc.at_cell(p, 5, -5, 4.5), pc.at_cell(p, 5, -5, -0.5)]
    got = sv.place_descriptor(**{k: v for k, v in pc.frame(sv, rows, p).items()})
    want = np.zeros((4, 8), np.uint8)
    want[0, 0], want[1, 2], want[2, 4], want[0, 7] = 128, 77, 77, 1  # (-600, -1): just below the negative x axis is sector 4; z_lo has code 1
    assert np.array_equal(got["desc"][0], want) and got["ring"][0].tolist() == [2, 1, 1, 0]
    assert got["words"][0].tolist() == [128 + 77 + 77 + 1, 4, 5, 3]  # dropped: the vehicle's own cell, beyond 1024 units, z_hi


def test_a_reciprocal_is_not_the_division(sv):
    case, differ = pc.near_integers(sv)
    assert differ >= 1  # floor(x * (1 / unit)) puts that many of these rows into another cell than floor(x / unit)
    assert pc.same(pc.call_descriptor(sv.place_descriptor_brute, case), pc.call_descriptor(sv.place_descriptor, case), pc.DESC_FIELDS)


def test_match_numpy_equals_brute(sv, match_all, match_wanted):
    for name, case in match_all.items():
        assert pc.same(pc.call_match(sv.place_match_brute, case, want_pair=True), match_wanted[name], pc.MATCH_FIELDS + ("pair",)), name


def test_match_by_hand(sv, match_wanted):
    w = match_wanted
    assert w["full"]["best"].tolist() == [[0, 0, 254 * 4096, 256 * 4096]] and w["constant"]["best"].tolist() == [[0, 0, 240, 1920]]
    assert w["tie"]["pair"].tolist() == [[[6, 0], [3, 0]]] and w["tie"]["best"].tolist() == [[0, 0, 6, 14]] and w["tie_swapped"]["best"].tolist() == [[0, 0, 3, 7]]
    assert w["close"]["best"].tolist() == [[1, 0, 3, 7]] and w["close"]["pair"][0, 0].tolist() == [5, 0]
    assert w["cross64"]["best"].tolist() == [[1, 0, 409598, 1228802]]
    assert w["gap"]["pair"][0, :, 0].tolist() == [0, 0, -1, -1, -1] and w["gap"]["counts"].tolist() == [[2, 2, 1]]
    assert w["gate_at"]["counts"].tolist() == [[1, 1, 1]] and w["gate_below"]["counts"].tolist() == [[1, 0, 0]] and w["gate_below"]["best"].tolist() == [list(sv.PLACE_NONE)]
    assert w["accept_at"]["best"].tolist() == [[0, 0, 6, 16]] and w["accept_below"]["best"].tolist() == [[-1, 0, 6, 16]] and w["accept_below"]["counts"].tolist() == [[1, 1, 0]]
    assert w["empty_query"]["best"].tolist() == [list(sv.PLACE_NONE), [0, 0, 0, 10]] and w["empty_key"]["counts"].tolist() == [[2, 2, 1]] and w["empty_key"]["best"][0, 0] == 3
    assert w["K0"]["best"].tolist() == [list(sv.PLACE_NONE)] and w["K0"]["pair"].shape == (1, 0, 2)


@pytest.mark.parametrize("S", [8, 60, 64, 128])
def test_a_rolled_descriptor_returns_its_shift(sv, S):
    rng = np.random.default_rng(S)
    d = rng.integers(0, 256, (1, 3, S)).astype(np.uint8)
    keys = np.repeat(d, 2, 0)
    q = np.concatenate([np.roll(d, -s, axis=2) for s in range(S)])  # q[c] = k[c + s]
    case = pc.match_case(q, keys)
    for f in (sv.place_match, sv.place_match_brute) if S <= 60 else (sv.place_match,):
        got = pc.call_match(f, case)
        assert got["best"][:, 0].tolist() == [0] * S and got["best"][:, 1].tolist() == list(range(S)) and (got["best"][:, 2] == 0).all()
    assert np.allclose(sv.place_yaw(np.arange(S), S), [2 * np.pi * (s if 2 * s <= S else s - S) / S for s in range(S)], atol=1e-15)


def test_yaw_and_guess(sv):
    assert sv.place_yaw(30, 60) == np.pi and sv.place_yaw(31, 60) < 0 and sv.place_yaw(0, 60) == 0
    g = sv.place_guess(sv.voxel_map_pose(3.0, -2.0, 3.0, 0.5), 5, 60)  # 3.0 + pi / 6 wraps
    assert g[:3].tolist() == [3.0, -2.0, 0.5] and abs(g[3] - (3.0 + np.pi / 6 - 2 * np.pi)) < 1e-12


@pytest.mark.parametrize("seed", TOWN_SEEDS)
def test_the_town_is_recognised(sv, seed):
    p = sv.place_params(pc.TOWN_R_MAX)
    world, places = pc.town(seed), pc.town_places()
    keys = [pc.seen_from(sv, world, p, x, y, 0.0) for x, y in places]
    assert min(n for _, n in keys) >= 200  # a few hundred rows each
    turn, x0, y0 = np.radians(30.0), places[20, 0], places[20, 1]
    truth = (x0 - 0.5 * np.sin(turn), y0 + 0.5 * np.cos(turn), turn)  # half a metre to the left of where it looks
    q, _ = pc.seen_from(sv, world, p, *truth)
    cat = lambda f: np.concatenate([k[f] for k, _ in keys])
    got = sv.place_match(q["desc"], q["words"], q["ring"], np.array([1000], np.int32), cat("desc"), cat("words"), cat("ring"), np.arange(41, dtype=np.int32), 50, want_pair=True)
    ratio = got["pair"][0, :, 0] / (q["words"][0, 0] + cat("words")[:, 0])
    order = np.argsort(ratio)
    print("seed %d: right key %.3f, runner-up %.3f (key %d), shift %d" % (seed, ratio[20], ratio[order[1]], order[1], got["best"][0, 1]))
    assert got["best"][0, 0] == 20 and order[0] == 20
    assert ratio[order[1]] >= TOWN_MARGIN * ratio[20]
    assert abs(sv.place_yaw(got["best"][0, 1], 60) - turn) <= 2 * np.pi / 60  # within one sector
    guess = sv.place_guess(sv.voxel_map_pose(x0, y0, 0.0), got["best"][0, 1], 60)
    assert abs(guess[0] - truth[0]) <= LOCALIZE_HALF[0] and abs(guess[1] - truth[1]) <= LOCALIZE_HALF[1] and abs(guess[3] - truth[2]) <= LOCALIZE_HALF[2]


def _loop(sv, frames=30):
    """A drive once round a block of the town and on into the first street again: poses, and the rows seen at each."""
    world = pc.town(7)
    t = np.arange(frames) * (2 * np.pi / (frames - 5))
    x, y, yaw = 80 + 25 * np.cos(t), 80 + 25 * np.sin(t), t + np.pi / 2
    rows = []
    for k in range(frames):
        near = world[(np.abs(world[:, 0] - x[k]) < 45) & (np.abs(world[:, 1] - y[k]) < 45)]
        rows.append(near)
    cap = max(len(r) for r in rows)
    xyz = np.full((frames, cap, 3), np.nan, np.float32)
    for k, r in enumerate(rows):
        xyz[k, :len(r)] = r
    return xyz, np.array([len(r) for r in rows], np.int32), sv.voxel_map_pose(x, y, yaw)


def _drive_index(sv, device, xyz, counts, poses, capacity=4):
    """Every frame described, searched among the frames at least 20 before it, then stored: an index that grows from `capacity`."""
    import torch
    rig = util.pkg("rig")
    index = rig.PlaceIndex(sv.place_params(pc.TOWN_R_MAX), capacity, device=device)
    to = (lambda a: torch.from_numpy(a).to(device))
    found = []
    for k in range(len(xyz)):
        d = index.descriptor(to(xyz[k:k + 1]), None, to(counts[k:k + 1]), sv.voxel_render_cams(poses[k:k + 1]))
        if index.count:
            res = index.query(d, k, 20, accept=128, want_pair=True)
            ok, guess = index.guess(res)
            found.append({"best": res["best"].cpu().numpy(), "counts": res["counts"].cpu().numpy(), "pair": res["pair"].cpu().numpy(), "ok": ok, "guess": guess})
        index.add(d, k, poses[k:k + 1])
    return index, found


def test_place_index_on_cpu_tensors(sv):
    xyz, counts, poses = _loop(sv)
    index, found = _drive_index(sv, "cpu", xyz, counts, poses)
    assert index.count == 30 and index.capacity == 32 and index.seq[:30].tolist() == list(range(30))  # 4 -> 8 -> 16 -> 32
    assert np.array_equal(index.poses[:30].numpy(), poses)
    again = sv.place_descriptor(xyz[3:4], None, counts[3:4], index.params, sv.voxel_render_cams(poses[3:4]))
    assert np.array_equal(index.desc[3].numpy(), again["desc"][0]) and np.array_equal(index.words[3].numpy(), again["words"][0])  # kept across the copies
    assert all(f["counts"][0, 0] == max(0, k + 1 - 20) for k, f in enumerate(found, 1))
    last = found[-1]  # frame 29 stands where frame 4 stood
    assert last["ok"][0] and last["best"][0, 0] == 4 and last["best"][0, 1] == 0
    want = sv.place_guess(poses[4], 0, 60)
    assert np.array_equal(last["guess"][0], want)
    assert not found[5]["ok"][0] and np.isnan(found[5]["guess"]).all()  # nothing 20 frames back yet


# ---------------------------------------------------------------------------------------------------------------- GPU

def _garbage(res):
    for t in res.values():
        t.fill_(0x5A)


@pytest.mark.gpu
def test_gpu_descriptor_equals_numpy(sv, eng, desc_cases, desc_wanted):
    import torch
    for name, case in desc_cases.items():
        dev = {k: None if case[k] is None else _cuda(case[k]) for k in ("xyz", "n", "counts")}
        got = eng.place_descriptor(dev["xyz"], dev["n"], dev["counts"], case["params"], case["poses"])
        _garbage(got)
        again = eng.place_descriptor(dev["xyz"], dev["n"], dev["counts"], case["params"], case["poses"], out=got)  # into buffers full of garbage
        assert again is got
        host = {k: v.cpu().numpy() for k, v in got.items()}
        assert pc.same(host, desc_wanted[name], pc.DESC_FIELDS), (name, [int((host[k] != desc_wanted[name][k]).sum()) for k in pc.DESC_FIELDS])
        if case["n"] is not None:  # and without weights
            bare = eng.place_descriptor(dev["xyz"], None, dev["counts"], case["params"], case["poses"])
            want = sv.place_descriptor(case["xyz"], None, case["counts"], case["params"], case["poses"])
            assert pc.same({k: v.cpu().numpy() for k, v in bare.items()}, want, pc.DESC_FIELDS), name
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_match_equals_numpy(sv, eng, match_all, match_wanted):
    for name, case in match_all.items():
        args = [_cuda(a) for a in case["args"][:8]] + [case["args"][8]]
        got = eng.place_match(*args, **case["words"], want_pair=True)
        host = {k: v.cpu().numpy() for k, v in got.items()}
        assert pc.same(host, match_wanted[name], pc.MATCH_FIELDS + ("pair",)), (name, host["best"].tolist(), match_wanted[name]["best"].tolist())
        _garbage(got)
        bare = {k: got[k] for k in pc.MATCH_FIELDS}
        assert eng.place_match(*args, **case["words"], out=bare) is bare  # without pair, into garbage
        assert pc.same({k: v.cpu().numpy() for k, v in bare.items()}, match_wanted[name], pc.MATCH_FIELDS), name
        eng.debug_place(1)
        try:
            one = eng.place_match(*args, **case["words"], want_pair=True)
        finally:
            eng.debug_place(0)
        assert pc.same({k: v.cpu().numpy() for k, v in one.items()}, match_wanted[name], pc.MATCH_FIELDS + ("pair",)), name


@pytest.mark.gpu
@pytest.mark.parametrize("S", [8, 60, 64, 68, 128])
def test_gpu_a_rolled_descriptor_returns_its_shift(sv, eng, S):
    rng = np.random.default_rng(S)
    d = rng.integers(0, 256, (1, 3, S)).astype(np.uint8)
    case = pc.match_case(np.concatenate([np.roll(d, -s, axis=2) for s in range(S)]), np.repeat(d, 2, 0))
    got = eng.place_match(*[_cuda(a) for a in case["args"][:8]], 0)["best"].cpu().numpy()
    assert got[:, 0].tolist() == [0] * S and got[:, 1].tolist() == list(range(S)) and (got[:, 2] == 0).all()


@pytest.mark.gpu
def test_gpu_refusals(sv, eng):
    import ctypes
    import torch
    L = eng.place_lib()
    spec = eng.place_spec(sv.place_params(30.0))
    need = ctypes.c_size_t()
    assert L.sv_place_descriptor_workspace(2, 20, 60, ctypes.byref(need)) == 0 and need.value == 2 * 1204 * 4
    assert L.sv_place_match_workspace(3, 65, ctypes.byref(need)) == 0 and need.value == 3 * 2 * 32
    assert L.sv_place_match_workspace(65536, 1, ctypes.byref(need)) == -1 and L.sv_place_match_workspace(1, 2 ** 20 + 1, ctypes.byref(need)) == -1
    assert L.sv_place_descriptor_workspace(65536, 20, 60, ctypes.byref(need)) == -1 and L.sv_place_descriptor_workspace(1, 20, 62, ctypes.byref(need)) == -1
    assert L.sv_debug_place(2) == -1 and L.sv_debug_place(0) == 0
    t = torch.zeros(4096, dtype=torch.int32, device="cuda")
    p = t.data_ptr()
    spec.reserved[3] = 1
    assert L.sv_place_descriptor_device(p, 0, None, p, None, 1, 4, p, ctypes.byref(spec), p + 1024, p + 8192, p + 9000, p + 12000, 4816, None) == -1
    assert b"reserved" in eng.lib().sv_last_error(None)
    spec.reserved[3] = 0
    assert L.sv_place_descriptor_device(p, 0, None, p, None, 1, 4, p, ctypes.byref(spec), p + 1024, p + 8192, p + 9000, p + 12000, 4815, None) == -1  # the workspace
    assert L.sv_place_descriptor_device(p, 0, None, p, None, 1, 4, p, ctypes.byref(spec), p + 1022, p + 8192, p + 9000, p + 12000, 4816, None) == -1  # alignment
    assert L.sv_place_descriptor_device(p, 0, None, p, None, 1, 4, p, ctypes.byref(spec), p + 8, p + 8192, p + 9000, p + 12000, 4816, None) == -1  # desc over xyz
    assert L.sv_place_descriptor_device(None, 0, None, None, None, 0, 4, None, ctypes.byref(spec), None, None, None, None, 0, None) == 0  # B = 0
    torch.cuda.synchronize()
    assert int(t.abs().sum()) == 0  # nothing was enqueued


@pytest.mark.gpu
def test_gpu_place_index_equals_the_cpu_index(sv, eng):
    xyz, counts, poses = _loop(sv)
    on_cpu, want = _drive_index(sv, "cpu", xyz, counts, poses)
    on_gpu, got = _drive_index(sv, "cuda", xyz, counts, poses)
    assert on_gpu.count == on_cpu.count == 30 and on_gpu.capacity == 32
    for f in ("desc", "ring", "words", "seq", "poses"):
        assert np.array_equal(getattr(on_gpu, f)[:30].cpu().numpy(), getattr(on_cpu, f)[:30].numpy()), f
    for k, (g, w) in enumerate(zip(got, want)):
        assert all(np.array_equal(g[f], w[f], equal_nan=f == "guess") for f in g), k


@pytest.mark.gpu
def test_gpu_cli_places(sv, eng, tmp_path):
    from PIL import Image
    from test_occupancy_map import _drive_frames
    ls, rs = _drive_frames(3)
    for sub, frames in (("image_02", ls), ("image_03", rs)):
        os.makedirs(tmp_path / "kitti" / sub)
        for i in range(3):
            Image.fromarray(frames[i]).save(tmp_path / "kitti" / sub / ("%010d.png" % i))
    with open(tmp_path / "poses.txt", "w") as f:
        f.write("0.0 0.0 0.0\n1.15 0.0 0.0\n2.3 0.01 0.0\n")
    base = ["-k", str(tmp_path / "kitti"), "--batch", "2", "--ply", str(tmp_path / "ply"), "--voxel", "0.2", "--poses", str(tmp_path / "poses.txt"),
            "--voxel-map", str(tmp_path / "map.ply")]
    far, own = str(tmp_path / "far.txt"), str(tmp_path / "own.txt")
    sv.main(base + ["--places", far])  # three frames close no loop: an empty file
    assert open(far).read() == ""
    sv.main(base + ["--places", own + ",0,256"])  # with no gap every frame finds itself
    lines = [line.split() for line in open(own)]
    assert [(int(w[0]), int(w[1]), int(w[2]), int(w[3])) for w in lines] == [(0, 0, 0, 0), (1, 1, 0, 0), (2, 2, 0, 0)]
    assert all(len(w) == 6 and int(w[4]) > 0 and float(w[5]) == 0.0 for w in lines)
    for bad in (",3","x.txt,-1", "x.txt,1,2,3", "x.txt,a"):
        with pytest.raises(SystemExit):
            sv.main(base + ["--places", bad])
    with pytest.raises(SystemExit):
        sv.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--places", far])  # needs --voxel-map
