"""The temporal warp of disparity maps (group (AA)): stereo_vision.sv.disparity_warp against numbers worked out by hand on painted maps
(warp_cases.py) and against its pixel-by-pixel form, on two KITTI frames under the fitted motion, and the GPU path - shape, dtype and
bits - against the numpy form."""
import os

import numpy as np
import pytest

import flow_cases as fc
import util
import warp_cases as wc
from flow_cases import IDENTITY, KITTI, SMALL
from test_top_view import _cuda, eng, sv  # noqa: F401 (fixtures)
from warp_cases import H, W, same

SV_ERR_ARG = -1
KITTI_GUESS = fc.pose_of(np.eye(3), (0.0, 0.0, -1.16))


def _both(sv, d_prev, d_cur, cam, poses, **words):
    """The numpy form, after it has been held against the brute form."""
    got = sv.disparity_warp(d_prev, d_cur, cam, poses, **words)
    want = sv.disparity_warp_brute(d_prev, d_cur, cam, poses, **words)
    assert same(got, want), wc.differences(got, want)
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_identity(sv):
    d = wc.identity_case()
    got = _both(sv, d[None], d[None], SMALL, IDENTITY[None])
    d0q = np.where(d > 0, np.floor(16.0 * d.astype(np.float64) + 0.5), 0).astype(np.int32)
    index = np.arange(H * W, dtype=np.int32).reshape(H, W)
    assert np.array_equal(got["expected"][0], d0q) and d0q[0, 0] == 960 and d0q[H - 1, W - 1] == 1
    assert np.array_equal(got["source"][0], np.where(d0q > 0, index, -1))
    assert np.array_equal(got["label"][0], np.where(d0q > 0, 3, 0)) and _bits(got["out"]).tobytes() == _bits(d).tobytes()
    n = int((d0q > 0).sum())
    assert got["counts"].tolist() == [[n, n, H * W - n, 0, 0, n, 0, 0]] and 0 < n < H * W


@pytest.mark.parametrize("case", wc.painted(), ids=lambda c: c["name"])
def test_painted_by_hand(sv, case):
    got = _both(sv, case["d_prev"][None], case["d_cur"][None], SMALL, case["pose"][None], **case["words"])
    expected, source = np.zeros((H, W), np.int32), np.full((H, W), -1, np.int32)
    for (v, u), (ex, src) in case["want"].items():
        expected[v, u], source[v, u] = ex, src
    assert np.array_equal(got["expected"][0], expected), (got["expected"][0].nonzero(), case["want"])
    assert np.array_equal(got["source"][0], source)
    assert got["counts"][0, :2].tolist() == [case["kept"], case["covered"]] and got["counts"][0, 2:].sum() == H * W
    # outputs in full: where nothing is expected the labels are 0 and 1 and the filled map is the measured one
    mq = sv._flow_dq(case["d_cur"])
    nothing = expected == 0
    assert np.array_equal(got["label"][0][nothing], np.where(mq > 0, 1, 0)[nothing])
    assert np.array_equal(_bits(got["out"][0])[nothing], np.where(mq > 0, _bits(case["d_cur"]), wc.NONE_BITS)[nothing])


@pytest.mark.parametrize("rel_q", [0, 64])
def test_tolerance_edge(sv, rel_q):
    d_cur, t, labels = wc.threshold_case(rel_q)
    assert t == (16, 48)[rel_q == 64]
    got = _both(sv, wc.blank(8.0)[None], d_cur[None], SMALL, IDENTITY[None], rel_q=rel_q)
    assert (got["expected"] == 128).all() and got["label"][0, 0, :4].tolist() == list(labels) and (got["label"][0, 1:] == 3).all()
    assert got["counts"][0].tolist() == [H * W, H * W, 0, 0, 0, H * W - 2, 1, 1]


def test_modes(sv):
    d_prev, d_cur, labels = wc.modes_case()
    none, fill = wc.NONE_BITS, int(_bits(np.float32(133.0 / 16.0).reshape(1))[0])
    own = [int(v) for v in _bits(d_cur[0, :6])]
    assert own[3] != int(_bits(np.float32(8.0).reshape(1))[0])  # not a multiple of 1/16: the bits are d_cur's, not a rounded value's
    want = {"fill": [none, own[1], fill, own[3], own[4], own[5]], "confirm": [none, none, none, own[3], none, none], "reject": [none, own[1], none, own[3], none, none]}
    for mode, row in want.items():
        got = _both(sv, d_prev[None], d_cur[None], SMALL, IDENTITY[None], mode=mode)
        assert got["label"][0, 0, :6].tolist() == list(labels) and got["expected"][0, 0, :6].tolist() == [0, 0, 133, 128, 128, 128]
        assert [int(v) for v in _bits(got["out"][0, 0, :6])] == row, mode
        assert (got["label"][0, 1:] == 0).all() and (_bits(got["out"][0, 1:]) == none).all()
        assert got["counts"][0].tolist() == [4, 4, H * W - 5, 1, 1, 1, 1, 1]
        assert same(sv.disparity_warp(d_prev[None], d_cur[None], SMALL, IDENTITY[None], mode=sv.WARP_MODES[mode]), got)


def test_without_a_current_map(sv):
    for case in wc.painted():
        got = _both(sv, case["d_prev"][None], None, SMALL, case["pose"][None], **case["words"])
        full = sv.disparity_warp(case["d_prev"][None], case["d_cur"][None], SMALL, case["pose"][None], **case["words"])
        assert got["label"] is None and got["out"] is None and same(got, full, ("expected", "source"))
        reached = int((got["expected"] > 0).sum())
        assert got["counts"][0].tolist() == full["counts"][0, :2].tolist() + [H * W - reached, 0, reached, 0, 0, 0]


def test_words_and_arguments(sv):
    assert sv.warp_words() == dict(e_max=1, tol_q=16, rel_q=0, mode=0) and sv.warp_words(4, 2 ** 20, 256, "reject") == dict(e_max=4, tol_q=2 ** 20, rel_q=256, mode=2)
    assert sv.warp_words(0, 0, 0, 1)["mode"] == 1
    for bad in (dict(e_max=-1), dict(e_max=5), dict(e_max=1.0), dict(e_max=True), dict(tol_q=-1), dict(tol_q=2 ** 20 + 1), dict(tol_q=None), dict(rel_q=-1), dict(rel_q=257),
                dict(rel_q="0"), dict(mode="keep"), dict(mode=3), dict(mode=-1), dict(mode=None), dict(mode=True), dict(mode=1.0)):
        with pytest.raises(ValueError):
            sv.warp_words(**bad)
    d = wc.blank(8.0)[None]

    def run(f, **bad):
        kw = dict(dict(d_prev=d, d_cur=d, camera=SMALL, poses=IDENTITY[None]), **bad)
        return f(kw.pop("d_prev"), kw.pop("d_cur"), kw.pop("camera"), kw.pop("poses"), **kw)

    for f in (sv.disparity_warp, sv.disparity_warp_brute):
        assert same(run(f), run(sv.disparity_warp))
        for bad in (dict(d_prev=d.astype(np.float64)), dict(d_prev=d[0]), dict(d_cur=d[:, 1:]), dict(d_cur=d.astype(np.int32)), dict(poses=IDENTITY), dict(poses=np.zeros((2, 12))),
                    dict(camera=dict(SMALL, f=0.0)), dict(camera=dict(SMALL, q32=float("nan"))), dict(e_max=9)):
            with pytest.raises(ValueError):
                run(f, **bad)
    empty = sv.disparity_warp(np.zeros((0, 3, 4), np.float32), None, SMALL, np.zeros((0, 12)))
    assert empty["expected"].shape == (0, 3, 4) and empty["counts"].shape == (0, 8)


@pytest.mark.parametrize("seed", range(4))
def test_random_maps_against_the_brute_form(sv, seed):
    d_prev, d_cur, poses, cam = wc.random_case(seed)
    got = _both(sv, d_prev, d_cur, cam, poses, e_max=seed, tol_q=8 * seed, rel_q=32 * seed, mode=seed % 3)
    assert got["counts"][0, 0] > 300 and (got["counts"][0, 2:] > 0).sum() >= 5  # the case is not empty: most labels occur


def test_cpu_tensors_take_the_numpy_form(sv):
    import torch
    engine = util.pkg("engine")
    d_prev, d_cur, poses, cam = wc.random_case(1)
    got = engine.disparity_warp(torch.from_numpy(d_prev), torch.from_numpy(d_cur), cam, poses, e_max=2)
    assert same({k: getattr(got, k) for k in wc.FIELDS}, sv.disparity_warp(d_prev, d_cur, cam, poses, e_max=2))


@pytest.fixture(scope="module")
def kitti_d1():
    """D1 of kitti0 and kitti1 from the oracle on the CPU at disp_max = 127, with the left images (test_flow.py's way)."""
    from pyoracle import ElasParams, Oracle
    L = [util.load_png("kitti%d_left.png" % k) for k in range(2)]
    R = [util.load_png("kitti%d_right.png" % k) for k in range(2)]
    return L, [Oracle().process(ElasParams.driver(127), l, r)[0] for l, r in zip(L, R)]


def test_kitti_pair(sv, kitti_d1):
    """kitti0 -> kitti1 at e_max = 1, tol_q = 16, rel_q = 0: under the fitted motion more pixels agree with the frame before than under the
    identity, and fewer than 5 % of the pixels have a measurement and no prediction.  A prototype of the definition gave 287398 against
    213846 pixels that agree, and 11169 of 465750 measured only."""
    L, D = kitti_d1
    m = sv.flow_match(L[0][None], L[1][None], D[0][None], D[1][None], KITTI, KITTI_GUESS[None], step=16, r=4, wx=8, wy=8, capacity=4096)
    fit = sv.flow_egomotion(m["matches"], m["counts"], KITTI, KITTI_GUESS[None])
    assert fit["ok"].all()
    moved = sv.disparity_warp(D[0][None], D[1][None], KITTI, fit["poses"], e_max=1, tol_q=16, rel_q=0)["counts"][0]
    still = sv.disparity_warp(D[0][None], D[1][None], KITTI, IDENTITY[None], e_max=1, tol_q=16, rel_q=0)["counts"][0]
    print("fitted:   " + sv.cli_temporal_text(moved))
    print("identity: " + sv.cli_temporal_text(still))
    assert moved[5] > still[5]
    assert moved[3] < 0.05 * D[1].size


def test_header_build_and_loader_agree(sv):
    text = open(os.path.join(util.ROOT, "include", "stereo_vision_hip.h")).read()
    for name in ("sv_disparity_warp_workspace", "sv_disparity_warp_device", "sv_warp_spec"):
        assert name in text
    assert "(AA) Behind the engine" in text and text.index("/* ---- (Z)") < text.index("/* ---- (AA)") < text.index("/* ---- (A)")
    build = util.pkg("build")
    assert "warp_kernels.hip" in build.SOURCES and "warp.cpp" in build.SOURCES and "warp_kernels.h" in build.HEADERS and "flow_point.h" in build.HEADERS
    engine = util.pkg("engine")
    assert set(engine.STAGE_SIGNATURES["warp"]) == {"sv_disparity_warp_workspace", "sv_disparity_warp_device"}
    import ctypes
    assert ctypes.sizeof(engine.SvWarpSpec) == 6 * 8 + 16 * 4
    for argv in (["--temporal", "out"], ["--batch", "2", "--temporal", "out"], ["--batch", "2", "--odometry", "p.txt", "--temporal", "out,x"],
                 ["--batch", "2", "--odometry", "p.txt", "--temporal", "out,1,keep"], ["--batch", "2", "--odometry", "p.txt", "--temporal", ",1"]):
        with pytest.raises(SystemExit):
            sv.main(["-k", "nowhere"] + argv)
    assert sv.cli_temporal_spec("out") == ("out", 16, "fill") and sv.cli_temporal_spec("out,0.5,confirm") == ("out", 8, "confirm")


# ---------------------------------------------------------------------------------------------------------------- GPU

def _gpu(eng, d_prev, d_cur, cam, poses, **kw):
    res = eng.disparity_warp(_cuda(d_prev), None if d_cur is None else _cuda(d_cur), cam, poses, **kw)
    return {k: None if getattr(res, k) is None else getattr(res, k).cpu().numpy() for k in wc.FIELDS}


def _agree(sv, eng, d_prev, d_cur, cam, poses, **words):
    got, want = _gpu(eng, d_prev, d_cur, cam, poses, **words), sv.disparity_warp(d_prev, d_cur, cam, poses, **words)
    assert same(got, want), wc.differences(got, want)
    return want


@pytest.mark.gpu
def test_gpu_painted_set(sv, eng):
    """The painted frames, those of equal words in one batch, with a current map and without one."""
    cases = wc.painted()
    d, dc, labels = wc.modes_case()
    cases += [dict(d_prev=d, d_cur=dc, pose=IDENTITY, words=dict(mode=mode)) for mode in ("fill", "confirm", "reject")]
    cases += [dict(d_prev=wc.blank(8.0), d_cur=wc.threshold_case(rel_q)[0], pose=IDENTITY, words=dict(rel_q=rel_q)) for rel_q in (0, 64)]
    cases.append(dict(d_prev=wc.identity_case(), d_cur=wc.identity_case(), pose=IDENTITY, words={}))
    groups = {}
    for c in cases:
        groups.setdefault(tuple(sorted(c["words"].items())), []).append(c)
    assert len(groups[()]) >= 12
    for words, group in groups.items():
        d_prev, d_cur, poses = (np.stack([c[k] for c in group]) for k in ("d_prev", "d_cur", "pose"))
        _agree(sv, eng, d_prev, d_cur, SMALL, poses, **dict(words))
        _agree(sv, eng, d_prev, None, SMALL, poses, **dict(words))


@pytest.mark.gpu
@pytest.mark.parametrize("h", [1, 5, 70])
@pytest.mark.parametrize("w", [1, 63, 64, 65, 67, 130])
def test_gpu_odd_shapes(sv, eng, w, h):
    d_prev, d_cur, poses, cam = wc.random_case(w + h, (h, w), cam=SMALL)
    want = _agree(sv, eng, d_prev, d_cur, cam, poses, e_max=2, rel_q=16)
    assert want["counts"][0, 0] > 0 or h * w < 60


@pytest.mark.gpu
def test_gpu_batch_of_three(sv, eng):
    d_prev, d_cur, poses, cam = wc.random_case(11, (70, 67), B=3, cam=SMALL)
    poses[1] = wc.translate(tz=-1.0)
    want = _agree(sv, eng, d_prev, d_cur, cam, poses, e_max=1, mode="reject")
    assert len({tuple(c) for c in want["counts"].tolist()}) == 3 and (want["counts"][:, 0] > 1000).all()
    for b in range(3):  # a frame of the batch is the frame alone
        assert same({k: v[b:b + 1] for k, v in want.items()}, sv.disparity_warp(d_prev[b:b + 1], d_cur[b:b + 1], cam, poses[b:b + 1], e_max=1, mode="reject"))


@pytest.mark.gpu
def test_gpu_a_wavefront_on_one_pixel(sv, eng):
    """64 sources in a row, u = 0 .. 63 with 64 - u px, under the sideways motion that moves each by its disparity: all to column 64."""
    cam = dict(SMALL, width=70, height=3, cx=35.0, cy=1.0)
    d = np.full((1, 3, 70), -1.0, np.float32)
    d[0, 1, :64] = 64.0 - np.arange(64)
    want = _agree(sv, eng, d, wc.noise(3, shape=(1, 3, 70)), cam, wc.translate(tx=0.5)[None])
    assert want["counts"][0, :2].tolist() == [64, 64] and (want["expected"] > 0).sum() == 1 and want["expected"][0, 1, 64] == 1024 and want["source"][0, 1, 64] == 70


@pytest.mark.gpu
def test_gpu_wide_covers_across_tiles(sv, eng):
    """Far points under a long step forward: covers of up to 5 x 5 that reach into the rows - and so the workgroups' tiles of 256 pixels -
    below them."""
    cam = dict(SMALL, width=67, height=70, cx=33.2, cy=35.3)
    d_prev = wc.noise(21, 1.0, 4.0, 0.1, (2, 70, 67))
    d_cur = wc.noise(22, 1.0, 20.0, 0.2, (2, 70, 67))
    poses = np.stack([wc.translate(tz=-4.0), wc.translate(0.1, -0.05, -4.2)])
    want = _agree(sv, eng, d_prev, d_cur, cam, poses, e_max=4)
    assert (want["counts"][:, 1] > sv.disparity_warp(d_prev, d_cur, cam, poses, e_max=3)["counts"][:, 1]).all()  # covers of 5 x 5 are there
    _agree(sv, eng, d_prev, d_cur, cam, poses, e_max=0)


@pytest.mark.gpu
def test_gpu_dirty_buffers(sv, eng):
    import torch
    d_prev, d_cur, poses, cam = wc.random_case(5, (70, 65), B=2, cam=SMALL)
    shape = d_prev.shape
    out = eng.WarpResult(expected=torch.full(shape, 0x7F7F7F7F, dtype=torch.int32, device="cuda"), source=torch.full(shape, 12345, dtype=torch.int32, device="cuda"),
                         label=torch.full(shape, 9, dtype=torch.uint8, device="cuda"), out=torch.full(shape, float("nan"), dtype=torch.float32, device="cuda"),
                         counts=torch.full((2, 8), -77, dtype=torch.int32, device="cuda"))
    ws = torch.full((2 * 70 * 65,), -1, dtype=torch.int64, device="cuda")  # all ones: a key that was not cleared would win every pixel
    want = sv.disparity_warp(d_prev, d_cur, cam, poses, e_max=2)
    for _ in range(2):  # the second call finds the first one's keys and counts
        res = eng.disparity_warp(_cuda(d_prev), _cuda(d_cur), cam, poses, e_max=2, out=out, workspace=ws)
        assert res is out
        got = {k: getattr(res, k).cpu().numpy() for k in wc.FIELDS}
        assert same(got, want), wc.differences(got, want)


@pytest.mark.gpu
def test_gpu_argument_checks(eng):
    import ctypes
    import torch
    L = eng.warp_lib()
    good = eng.warp_spec(SMALL)
    n = H * W
    buf = torch.full((8 * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")  # d_prev, d_cur, expected, source, out, label + counts, 2 n of workspace
    base = buf.data_ptr()
    at = lambda k: base + 4 * n * k
    poses = torch.from_numpy(IDENTITY.copy()).cuda()
    need = ctypes.c_size_t(77)

    def call(spec=good, d_prev=at(0), d_cur=at(1), pose=poses.data_ptr(), batch=1, w=W, h=H, expected=at(2), source=at(3), label=at(5), out=at(4), counts=at(5) + n, ws=at(6),
             ws_bytes=8 * n):
        return L.sv_disparity_warp_device(d_prev, d_cur, pose, batch, w, h, None if spec is None else ctypes.byref(spec), expected, source, label, out, counts, ws, ws_bytes, None)

    for field, bad in (("e_max", -1), ("e_max", 5), ("tol_q", -1), ("tol_q", 2 ** 20 + 1), ("rel_q", -1), ("rel_q", 257), ("mode", -1), ("mode", 3), ("f", 0.0), ("b16", float("nan")),
                       ("fb", -1.0), ("fb16", 0.0), ("cx", float("inf")), ("cy", float("nan"))):
        spec = eng.warp_spec(SMALL)
        setattr(spec, field, bad)
        assert call(spec=spec) == SV_ERR_ARG, field
    spec = eng.warp_spec(SMALL)
    spec.reserved[11] = 1
    assert call(spec=spec) == SV_ERR_ARG
    for kw in (dict(spec=None), dict(d_prev=None), dict(pose=None), dict(expected=None), dict(source=None), dict(label=None), dict(out=None), dict(counts=None), dict(ws=None),
               dict(d_prev=at(0) + 2), dict(d_cur=at(1) + 1), dict(pose=poses.data_ptr() + 4), dict(expected=at(2) + 2), dict(source=at(3) + 1), dict(out=at(4) + 2),
               dict(counts=at(5) + n + 2), dict(ws=at(6) + 4), dict(ws_bytes=8 * n - 1), dict(batch=-1), dict(batch=65536), dict(w=0), dict(h=0), dict(w=8193), dict(h=8193),
               dict(out=at(1)), dict(expected=at(0)), dict(source=at(2)), dict(ws=at(3)), dict(counts=at(2))):
        assert call(**kw) == SV_ERR_ARG, kw
    assert L.sv_disparity_warp_workspace(W, H, 1, None) == SV_ERR_ARG and L.sv_disparity_warp_workspace(0, H, 1, ctypes.byref(need)) == SV_ERR_ARG
    assert L.sv_disparity_warp_workspace(W, 8193, 1, ctypes.byref(need)) == SV_ERR_ARG and L.sv_disparity_warp_workspace(W, H, 65536, ctypes.byref(need)) == SV_ERR_ARG
    assert need.value == 77 and L.sv_disparity_warp_workspace(W, H, 3, ctypes.byref(need)) == 0 and need.value == 3 * 8 * n
    assert call(batch=0, d_prev=None, d_cur=None, pose=None, expected=None, source=None, label=None, out=None, counts=None, ws=None, ws_bytes=0) == 0
    torch.cuda.synchronize()
    assert (buf == 0x5A5A5A5A).all()  # nothing was enqueued: no output and no byte of the workspace was touched
    buf[:2 * n] = torch.from_numpy(np.stack([wc.identity_case(), wc.identity_case()])).cuda().view(torch.int32).reshape(-1)
    assert call() == 0 and call(d_cur=None, label=None, out=None) == 0
    torch.cuda.synchronize()
    assert (buf[2 * n:3 * n] != 0x5A5A5A5A).all() and (buf[6 * n:] != 0x5A5A5A5A).all()


@pytest.fixture(scope="module")
def kitti_frames():
    ls = np.stack([np.repeat(util.load_png("kitti%d_left.png" % k)[..., None], 3, -1) for k in range(4)])
    rs = np.stack([np.repeat(util.load_png("kitti%d_right.png" % k)[..., None], 3, -1) for k in range(4)])
    return ls, rs


@pytest.mark.gpu
def test_gpu_rig_temporal(sv, eng, kitti_frames, tmp_path):
    """StereoRig.temporal on four KITTI frames: its own odometry, a caller's motions, a pair without a motion - against the numpy form on
    the same maps."""
    import torch
    ls, rs = kitti_frames
    yml = str(tmp_path / "rectified.yml")
    with open(yml, "w") as f:
        f.write(fc.RECTIFIED_YML)
    rig = util.pkg("rig").StereoRig(1242, 375, calibration=yml, params=eng.SvParams.driver(127))
    try:
        d1 = rig.disparity(ls, rs)
        camera = rig.render_camera(1.0)
        own = rig.temporal(torch.from_numpy(ls).cuda(), torch.from_numpy(rs).cuda())
        motions = np.tile(KITTI_GUESS, (3, 1))
        motions[1, 5] = np.nan  # the second pair has no motion
        given = rig.temporal(ls, rs, poses=motions, mode="confirm", tol_q=24, e_max=2)
        with pytest.raises(ValueError):
            rig.temporal(ls[:1], rs[:1])
        with pytest.raises(ValueError):
            rig.temporal(ls, rs, poses=motions[:2])
        with pytest.raises(ValueError):
            rig.temporal(ls, rs, mode="keep")
    finally:
        rig.close()
    assert own["ok"].all() and own["rel"].shape == (3, 12) and all(-1.25 <= t <= -1.08 for t in own["rel"][:, 11])
    want = sv.disparity_warp(d1[:-1], d1[1:], camera, own["rel"])
    got = {k: own[k].cpu().numpy() for k in ("label", "expected", "source", "counts")}
    got["out"] = own["d1"][1:].cpu().numpy()
    assert same(got, want), wc.differences(got, want)
    assert own["d1"][0].cpu().numpy().tobytes() == d1[0].tobytes()
    for k in range(3):
        print("kitti%d->%d: %s" % (k, k + 1, sv.cli_temporal_text(want["counts"][k])))  # printed only: the shares are the scene's, not the code's
    assert isinstance(given["label"], np.ndarray) and given["ok"].tolist() == [True, False, True]
    want = sv.disparity_warp(d1[:-1], d1[1:], camera, motions, mode="confirm", tol_q=24, e_max=2)
    want["out"][1] = d1[2]  # the pair without a motion keeps its measured map
    got = dict({k: given[k] for k in ("label", "expected", "source", "counts")}, out=given["d1"][1:])
    assert same(got, want), wc.differences(got, want)
    assert want["counts"][1, :2].tolist() == [0, 0] and set(np.unique(want["label"][1])) == {0, 1}


@pytest.mark.gpu
def test_gpu_cli(sv, eng, kitti_frames, tmp_path):
    from PIL import Image
    ls, rs = kitti_frames
    for sub, frames in (("image_02", ls), ("image_03", rs)):
        os.makedirs(tmp_path / "kitti" / sub)
        for i in range(4):
            Image.fromarray(frames[i]).save(tmp_path / "kitti" / sub / ("%010d.png" % i))
    poses, out, yml = str(tmp_path / "odo.txt"), str(tmp_path / "temporal"), str(tmp_path / "rectified.yml")
    with open(yml, "w") as f:
        f.write(fc.RECTIFIED_YML)
    sv.main(["-k", str(tmp_path / "kitti"), "--camera_calibration", yml, "--batch", "3", "--odometry", poses, "--temporal", out + ",1.5,reject"])
    rel = np.array([[float(w) for w in line.split()] for line in open(poses + ".rel.txt")])
    rig = util.pkg("rig").StereoRig(1242, 375, calibration=yml)  # the CLI's rig: the default parameters
    try:
        d1 = rig.disparity(ls, rs)  # gray frames: the channel order of the folder's PNGs does not matter
        camera = rig.render_camera(1.0)
    finally:
        rig.close()
    want = sv.disparity_warp(d1[:-1], d1[1:], camera, rel, tol_q=24, mode="reject")
    maps = np.concatenate([d1[:1], want["out"]])
    labels = np.concatenate([(sv._flow_dq(d1[:1]) > 0).astype(np.uint8), want["label"]])
    assert sorted(os.listdir(out)) == sorted("%06d.%s.png" % (i, kind) for i in range(4) for kind in ("change", "temporal"))
    for i in range(4):
        image = np.clip(np.rint(maps[i] * np.float32(4.0)), 0, 255).astype(np.uint8)  # the driver's 8-bit image: 4 d, half to even, saturated
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "%06d.temporal.png" % i))), image), i
        assert np.array_equal(np.asarray(Image.open(os.path.join(out, "%06d.change.png" % i))), sv.VOXEL_RENDER_PNG[labels[i]]), i
