"""The calibrated stereo rig (sv_rig_* / rig.StereoRig): calibration and maps on the host, the batched camera front end
(resize -> gray -> remap) against the numpy restatements of the legacy chain, the rig against the legacy entry, and the
rig's disparity / point clouds against the oracle."""
import ctypes
import os
import zlib

import numpy as np
import pytest

import util
from pyoracle import ElasParams
from test_legacy_entry import _gray_cv4, _remap_linear_u8, _resize_linear_8uc4

SV_ERR_ARG, SV_ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def rigmod():
    util.pkg("build").build()
    return util.pkg("rig")


def _yaml():
    return os.path.join(os.path.dirname(util.pkg("engine").LIB_PATH), "stereo_vision", "data", "kitti_2011_09_26.yml")


def _create(rigmod, path, w, h, rectify=0, scale=1.0, reserved=(0, 0, 0)):
    L = rigmod.rig_lib()
    cfg = rigmod.SvRigConfig(w, h, 0, rectify, scale)
    cfg.reserved[:] = list(reserved)
    r = ctypes.c_void_p()
    rc = L.sv_rig_create(path.encode() if path is not None else None, ctypes.byref(cfg), ctypes.byref(r))
    return rc, r, L


def _write_calibration(path, K, T, R=None, D=None, drop=None):
    R = np.eye(3) if R is None else R
    D = np.zeros(5) if D is None else D

    def mat(name, a, rows, cols):
        return "%s: !!opencv-matrix\n   rows: %d\n   cols: %d\n   dt: d\n   data: [ %s ]\n" % (name, rows, cols, ", ".join(repr(float(v)) for v in np.ravel(a)))

    parts = [("K1", K, 3, 3), ("D1", D, 1, 5), ("K2", K, 3, 3), ("D2", D, 1, 5), ("R", R, 3, 3), ("T", T, 3, 1)]
    with open(path, "w") as f:
        f.write("%YAML:1.0\n---\n")
        for name, a, r, c in parts:
            if name != drop:
                f.write(mat(name, a, r, c))
    return str(path)


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_rig_q_equals_stereo_rectify(rigmod):
    """Q of sv_rig_matrices == sv_debug_stereo_rectify's (the restatement the legacy entry used) bit for bit, scale 1 and 2."""
    yml = _yaml()
    for w, h, scale in ((1242, 375, 1.0), (621, 187, 2.0)):
        rc, r, L = _create(rigmod, yml, w, h, scale=scale)
        assert rc == 0
        try:
            Q = np.zeros(16)
            XR, XT = np.full(9, np.nan), np.full(3, np.nan)
            has = L.sv_rig_matrices(r, Q.ctypes.data, XR.ctypes.data, XT.ctypes.data)
        finally:
            L.sv_rig_destroy(r)
        L.sv_debug_stereo_rectify.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        Qd = np.zeros(16)
        assert L.sv_debug_stereo_rectify(yml.encode(), w, h, scale, 1, Qd.ctypes.data, None) == 0
        assert Q.tobytes() == Qd.tobytes()
        assert has in (0, 1, 2, 3) and ((has & 1) == 0) == bool(np.isnan(XR).all())
    rig = rigmod.StereoRig(1242, 375)
    try:
        assert rig.Q.shape == (4, 4) and rig.maps() is None and rig._engine is None
    finally:
        rig.close()


def test_rig_maps_identity_for_an_ideal_camera(rigmod, tmp_path):
    """No distortion, identity R, baseline along x: the rectification maps are the identity grid."""
    K = np.array([[100.0, 0, 32.0], [0, 100.0, 24.0], [0, 0, 1]])
    path = _write_calibration(tmp_path / "ideal.yml", K, np.array([-0.5, 0, 0]))
    rig = rigmod.StereoRig(64, 48, calibration=path, rectify=True)
    try:
        m = rig.maps()
    finally:
        rig.close()
    jj, ii = np.meshgrid(np.arange(64), np.arange(48))
    assert m.shape == (4, 48, 64) and m.dtype == np.float32
    for s in (0, 2):
        assert np.abs(m[s] - jj).max() < 1e-3 and np.abs(m[s + 1] - ii).max() < 1e-3
    assert abs(rig.Q[3, 2] - 2.0) < 1e-12  # -1 / Tx


def test_rig_rejects_bad_arguments(rigmod, tmp_path):
    yml = _yaml()
    K = np.array([[100.0, 0, 32.0], [0, 100.0, 24.0], [0, 0, 1]])
    no_t = _write_calibration(tmp_path / "no_t.yml", K, np.array([-0.5, 0, 0]), drop="T")
    cases = [(str(tmp_path / "missing.yml"), {}, "cannot open"), (no_t, {}, "T"), (yml, {"scale": 0.0}, "scale"), (yml, {"scale": -1.0}, "scale"),
             (yml, {"w": 31}, "size"), (yml, {"reserved": (0, 7, 0)}, "reserved")]
    for path, kw, word in cases:
        rc, r, L = _create(rigmod, path, kw.get("w", 1242), 375, scale=kw.get("scale", 1.0), reserved=kw.get("reserved", (0, 0, 0)))
        assert rc == SV_ERR_ARG and not r.value, (path, kw)
        assert word in L.sv_rig_last_error(None).decode(), (word, L.sv_rig_last_error(None))
    with pytest.raises(ValueError, match="scale"):
        rigmod.StereoRig(1242, 375, scale=0)
    # front-end arguments are checked before any device is touched
    rc, r, L = _create(rigmod, yml, 1242, 375)
    assert rc == 0
    try:
        assert L.sv_rig_maps(r, np.zeros(1, np.float32).ctypes.data) == SV_ERR_STATE
        for fmt, sw, sh, pitch, word in ((7, 1242, 375, 4968, "format"), (-1, 1242, 375, 4968, "format"), (0, 8193, 8193, 4 * 8193, "2^26"),
                                         (1, 1242, 375, 1242 * 3 - 1, "pitch"), (0, 0, 375, 4968, "size")):
            assert L.sv_rig_frontend_device(r, 16, 16, 1, sw, sh, pitch, fmt, 16, 16, None, None) == SV_ERR_ARG
            assert word in L.sv_rig_last_error(r).decode()
    finally:
        L.sv_rig_destroy(r)


def test_colour_fixture_matches_gray_fixture():
    """The committed colour KITTI pair 0 (image_02 / image_03) and the committed gray pair are the same pixels: gray_cv4(colour) == gray."""
    for side in ("left", "right"):
        rgb = util.load_png("kitti0_color_%s.png" % side)
        assert rgb.shape == (375, 1242, 3) and (rgb[..., 0] != rgb[..., 2]).mean() > 0.5
        assert np.array_equal(_gray_cv4(rgb), util.load_png("kitti0_%s.png" % side))


# ---------------------------------------------------------------------------------------------------------------- GPU

def _colour_frames(B, seed, crop=None):
    """B distinct RGB frames from the colour fixture: seeded per-channel offsets (mod 256), optionally cropped [h, w]."""
    base = util.load_png("kitti0_color_left.png").astype(np.int64)
    rng = np.random.default_rng(seed)
    out = np.stack([((base + rng.integers(0, 256, 3)) % 256).astype(np.uint8) for _ in range(B)])
    if crop is not None:
        out = np.ascontiguousarray(out[:, :crop[0], :crop[1]])
    return out


def _as_format(rgb, fmt, seed=0):
    if fmt == "rgb":
        return np.ascontiguousarray(rgb)
    if fmt == "bgr":
        return np.ascontiguousarray(rgb[..., ::-1])
    if fmt == "bgra":
        alpha = np.random.default_rng(seed).integers(0, 256, rgb.shape[:-1] + (1,), dtype=np.uint8)
        return np.ascontiguousarray(np.concatenate([rgb[..., ::-1], alpha], -1))
    return _gray_cv4(rgb)


def _expected_gray(rgb, fmt, W, H, maps_xy):
    """The legacy chain in numpy: resize (per channel) -> gray -> remap."""
    x = rgb if fmt != "gray" else _gray_cv4(rgb)[..., None]
    if x.shape[:2] != (H, W):
        x = _resize_linear_8uc4(x, W, H)
    g = _gray_cv4(x) if fmt != "gray" else x[..., 0]
    return _remap_linear_u8(g, *maps_xy) if maps_xy is not None else g


def _to_device(a, pad=0):
    import torch
    t = torch.from_numpy(a).cuda()
    if not pad:
        return t
    shape = list(a.shape)
    shape[2] += pad
    big = torch.full(shape, 77, dtype=torch.uint8, device="cuda")
    big[:, :, :a.shape[2]] = t
    v = big[:, :, :a.shape[2]]
    assert not v.is_contiguous()
    return v


# (rig size, source size): no resize, exact 2x (INTER_AREA shortcut), non-integer factors
_SIZES = {"none": ((1242, 375), (1242, 375)), "2x": ((621, 187), (1242, 374)), "621x187": ((621, 187), (1242, 375)), "800x241": ((800, 241), (1242, 375))}


@pytest.mark.gpu
@pytest.mark.parametrize("rectify", [False, True])
@pytest.mark.parametrize("size", list(_SIZES))
@pytest.mark.parametrize("fmt", ["bgra", "bgr", "rgb", "gray"])
def test_frontend_matches_numpy_chain(rigmod, fmt, size, rectify):
    (W, H), (sw, sh) = _SIZES[size]
    B = 3 if size in ("none", "800x241") else 1
    pad = 3 if fmt in ("bgr", "gray") or size == "2x" else 0  # pitch-padded sources (unaligned rows for BGR / gray)
    rgb = _colour_frames(B, seed=zlib.crc32((fmt + size).encode()), crop=(sh, sw))
    rig = rigmod.StereoRig(W, H, rectify=rectify)
    try:
        maps = rig.maps()
        L, R = _as_format(rgb, fmt, 1), _as_format(rgb[:, ::-1].copy(), fmt, 2)
        gl, gr = rig.frontend(_to_device(L, pad), _to_device(R, pad), pixel_format=fmt)
        gl, gr = gl.cpu().numpy(), gr.cpu().numpy()
    finally:
        rig.close()
    assert gl.shape == (B, H, W)
    for b in range(B):
        want_l = _expected_gray(rgb[b], fmt, W, H, (maps[0], maps[1]) if rectify else None)
        want_r = _expected_gray(rgb[b, ::-1].copy(), fmt, W, H, (maps[2], maps[3]) if rectify else None)
        assert np.array_equal(gl[b], want_l), (fmt, size, rectify, b)
        assert np.array_equal(gr[b], want_r), (fmt, size, rectify, b)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 67])
def test_frontend_batch_sizes_and_layouts(rigmod, B):
    """B in {1, 67} on a small rig (resize 200x130 -> 96x64 with the remap), numpy input: every pair its own; the same image in
    the three colour layouts gives the same gray."""
    rgb = _colour_frames(B, seed=B, crop=(130, 200))
    rig = rigmod.StereoRig(96, 64, rectify=True, scale=1242 / 96)
    try:
        maps = rig.maps()
        outs = {fmt: rig.frontend(_as_format(rgb, fmt, 3), _as_format(rgb[:, :, ::-1].copy(), fmt, 4), pixel_format=fmt) for fmt in ("bgra", "bgr", "rgb")}
        assert isinstance(outs["bgr"][0], np.ndarray)
        gl1, _ = rig.frontend(_as_format(rgb, "bgr")[0], _as_format(rgb, "bgr")[0], pixel_format="bgr")  # one frame without B
    finally:
        rig.close()
    for fmt in ("bgra", "rgb"):
        assert np.array_equal(outs[fmt][0], outs["bgr"][0]) and np.array_equal(outs[fmt][1], outs["bgr"][1])
    gl, gr = outs["bgr"]
    assert gl.shape == (B, 64, 96) and np.array_equal(gl1[0], gl[0])
    for b in range(B):
        assert np.array_equal(gl[b], _expected_gray(rgb[b], "bgr", 96, 64, (maps[0], maps[1]))), b
        assert np.array_equal(gr[b], _expected_gray(rgb[b, :, ::-1].copy(), "bgr", 96, 64, (maps[2], maps[3]))), b


def _bgra(rgb):
    return np.ascontiguousarray(np.concatenate([rgb[..., ::-1], np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2))


@pytest.mark.gpu
@pytest.mark.parametrize("rectify", [False, True])
@pytest.mark.parametrize("resize", [False, True])
def test_rig_equals_legacy_entry(rigmod, rectify, resize):
    """The colour fixture through generatePointCloud / getColor and through a rig: gray, u8 map, points and colours bit-identical."""
    eng = util.pkg("engine")
    rgb_l, rgb_r = util.load_png("kitti0_color_left.png"), util.load_png("kitti0_color_right.png")
    W, H = (621, 187) if resize else (1242, 375)
    L = eng.lib()
    L.generatePointCloud.restype = ctypes.c_void_p
    L.generatePointCloud.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_bool, ctypes.c_bool, ctypes.c_bool,
                                     ctypes.c_bool, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    L.clean.restype = None
    L.getColor.restype = ctypes.POINTER(ctypes.c_ubyte)
    L.sv_legacy_set_rectify.argtypes = [ctypes.c_int]
    L.sv_legacy_last_gray.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.sv_legacy_last_dmap.restype = ctypes.POINTER(ctypes.c_ubyte)
    yml = _yaml().encode()
    a_l, a_r = _bgra(rgb_l), _bgra(rgb_r)
    L.sv_legacy_set_rectify(int(rectify))
    try:
        first = np.zeros((H, W, 4), np.uint8)
        assert L.generatePointCloud(first.ctypes.data, first.ctypes.data, yml, W, H, True, False, False, False, 1, 1, b"", b"", b"")  # freezes W x H
        p = L.generatePointCloud(a_l.ctypes.data, a_r.ctypes.data, yml, 1242, 375, True, False, False, False, 1, 1, b"", b"", b"")
        pts = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), shape=(H * W * 3,)).reshape(H, W, 3).copy()
        gl, gr = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
        assert L.sv_legacy_last_gray(gl.ctypes.data, gr.ctypes.data) == 0
        dmap = np.ctypeslib.as_array(L.sv_legacy_last_dmap(None, None), shape=(H, W)).copy()
        colors = np.ctypeslib.as_array(L.getColor(), shape=(H, W, 4)).copy()
    finally:
        L.clean()
        L.sv_legacy_set_rectify(0)
    rig = rigmod.StereoRig(W, H, rectify=rectify)
    try:
        rgl, rgr = rig.frontend(a_l, a_r, pixel_format="bgra")
        d1, rdmap, rpts, rcol = rig.point_clouds(a_l, a_r, pixel_format="bgra", colors=True)
    finally:
        rig.close()
    assert np.array_equal(rgl[0], gl) and np.array_equal(rgr[0], gr)
    assert (rdmap[0] > 0).mean() > 0.3 and np.array_equal(rdmap[0], dmap)
    assert rpts.shape == (1, H, W, 3) and np.array_equal(rpts[0], pts, equal_nan=True)
    assert np.array_equal(rcol[0], colors)


@pytest.mark.gpu
def test_rig_disparity_equals_oracle(rigmod, oracle):
    """rig.disparity on 5 colour pairs (the fixture, and gray goldens made colour with seeded per-channel offsets) == the oracle on
    gray_cv4 of the same frames, at tolerance 0."""
    rng = np.random.default_rng(11)
    ls, rs = [util.load_png("kitti0_color_left.png")], [util.load_png("kitti0_color_right.png")]
    for k in (1, 2, 3, 4):
        off = rng.integers(-40, 40, 3)
        for side, dst in (("left", ls), ("right", rs)):
            g = util.load_png("kitti%d_%s.png" % (k, side)).astype(np.int64)
            dst.append(np.clip(g[..., None] + off, 0, 255).astype(np.uint8))
    L, R = np.stack(ls), np.stack(rs)
    rig = rigmod.StereoRig(1242, 375)
    try:
        d1 = rig.disparity(_as_format(L, "bgr"), _as_format(R, "bgr"), pixel_format="bgr")
    finally:
        rig.close()
    assert d1.shape == (5, 375, 1242) and d1.dtype == np.float32
    for b in range(5):
        o1, _, _ = oracle.process(ElasParams.driver(255), _gray_cv4(L[b]), _gray_cv4(R[b]))
        assert np.array_equal(d1[b].view(np.uint32), o1.view(np.uint32)), b


@pytest.mark.gpu
def test_two_rigs_are_independent(rigmod, tmp_path):
    """Two calibrations (the bundled one, and a copy with another baseline) interleaved on one thread: each rig gives its own Q and
    points, equal to a fresh single rig's."""
    import re
    txt = open(_yaml()).read()
    m = re.search(r"\nT:[^\[]*\[([^\]]*)\]", txt)
    T = [float(v) for v in m.group(1).replace("\n", " ").split(",")]
    other = txt[:m.start(1)] + ", ".join(repr(v * 1.5) for v in T) + txt[m.end(1):]
    path2 = tmp_path / "wide.yml"
    path2.write_text(other)
    L, R = _as_format(_colour_frames(2, 5), "bgr"), _as_format(_colour_frames(2, 6), "bgr")
    a, b = rigmod.StereoRig(1242, 375, rectify=True), rigmod.StereoRig(1242, 375, calibration=str(path2), rectify=True)
    try:
        assert not np.array_equal(a.Q, b.Q)
        outs = []
        for _ in range(2):
            outs.append(a.point_clouds(L, R, pixel_format="bgr"))
            outs.append(b.point_clouds(L, R, pixel_format="bgr"))
    finally:
        a.close()
        b.close()
    for k, path in enumerate((_yaml(), str(path2))):
        fresh = rigmod.StereoRig(1242, 375, calibration=path, rectify=True)
        try:
            want = fresh.point_clouds(L, R, pixel_format="bgr")
        finally:
            fresh.close()
        for got in (outs[k], outs[k + 2]):
            for g, w in zip(got, want):
                assert np.array_equal(g, w, equal_nan=True), path
    assert not np.array_equal(outs[0][2], outs[1][2], equal_nan=True)


@pytest.mark.gpu
def test_frontend_on_torch_current_stream(rigmod):
    """Inputs written by a torch op on a non-default current stream, no explicit synchronisation: the results are those of the
    same inputs handed over at rest."""
    import torch
    rgb = _colour_frames(4, 9)
    L, R = _as_format(rgb, "bgra", 1), _as_format(rgb[:, ::-1].copy(), "bgra", 2)
    rig = rigmod.StereoRig(1242, 375, rectify=True)
    try:
        want_g = rig.frontend(L, R, pixel_format="bgra")
        want_d = rig.disparity(L, R, pixel_format="bgra")
        src_l, src_r = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            x = torch.randn(4096, 4096, device="cuda")
            for _ in range(4):
                x = x @ x  # keeps the stream busy while the host runs ahead
            left = torch.empty_like(src_l)
            right = torch.empty_like(src_r)
            left.copy_(src_l)
            right.copy_(src_r)
            gl, gr = rig.frontend(left, right, pixel_format="bgra")
            gl2, gr2 = gl.clone(), gr.clone()
            left2 = src_l.clone()
            right2 = src_r.clone()
            d1 = rig.disparity(left2, right2, pixel_format="bgra")
        torch.cuda.synchronize()
        del x
    finally:
        rig.close()
    assert np.array_equal(gl2.cpu().numpy(), want_g[0]) and np.array_equal(gr2.cpu().numpy(), want_g[1])
    assert np.array_equal(d1.cpu().numpy().view(np.uint32), want_d.view(np.uint32))


@pytest.mark.gpu
def test_cli_batch_writes_the_per_frame_maps(tmp_path):
    """`python -m ...stereo_vision --batch 2 --out DIR` over an image_02 / image_03 folder writes the maps the per-frame path
    (generatePointCloud, last_disparity_u8) computes for the same frames."""
    from PIL import Image
    svmod = util.pkg("stereo_vision")
    for d in ("image_02", "image_03"):
        os.makedirs(tmp_path / "kitti" / d)
    frames = [(util.load_png("kitti0_color_left.png"), util.load_png("kitti0_color_right.png"))]
    rng = np.random.default_rng(3)
    for k in (1, 2):
        off = rng.integers(-30, 30, 3)
        frames.append(tuple(np.clip(util.load_png("kitti%d_%s.png" % (k, s)).astype(np.int64)[..., None] + off, 0, 255).astype(np.uint8) for s in ("left", "right")))
    for i, (l, r) in enumerate(frames):
        Image.fromarray(l).save(tmp_path / "kitti" / "image_02" / ("%010d.png" % i))
        Image.fromarray(r).save(tmp_path / "kitti" / "image_03" / ("%010d.png" % i))
    svmod.main(["-k", str(tmp_path / "kitti"), "--batch", "2", "--out", str(tmp_path / "batch")])
    s = svmod.stereo_vision(objectTracking=False, width=1242, height=375)
    try:
        for i, (l, r) in enumerate(frames):
            s.generatePointCloud(l[..., ::-1], r[..., ::-1])
            want = s.last_disparity_u8()
            got = np.asarray(Image.open(tmp_path / "batch" / ("%010d.png" % i)))
            assert (want > 0).mean() > 0.3 and np.array_equal(got, want), i
    finally:
        s.close()
