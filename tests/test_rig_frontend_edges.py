"""The rig's camera front end (rig_kernels.hip through sv_rig_frontend_device) at the edges of its input space: row tails of
1 - 3 pixels, tiny and huge resize factors, near-2x sources, padded and misaligned source rows, every pixel format, pairs b > 0,
remap taps outside the source, and writes next to the outputs.  Every kernel result equals the numpy restatement of the legacy
chain bit for bit and lies within a stated bound of a plain float64 version of the same chain; the restatements themselves are
checked against float64 on the CPU."""
import zlib

import numpy as np
import pytest

import util
from pyoracle import ElasParams
from test_legacy_entry import _gray_cv4, _remap_linear_u8, _resize_linear_8uc4
from test_rig import _as_format, _create, _expected_gray, _write_calibration, _yaml
from test_top_view import _d1_points, _reproject_np

SV_OK, SV_ERR_ARG = 0, -1
FORMATS = ["bgra", "bgr", "rgb", "gray"]
_FMT = {"bgra": 0, "bgr": 1, "rgb": 2, "gray": 3}
_CH = {"bgra": 4, "bgr": 3, "rgb": 3, "gray": 1}

# Largest difference of each restatement from float64 (asserted on random data below):
RESIZE_BOUND = 1.0  # _resize_linear_8uc4 per channel: < 1 (0.81 seen); float32 coordinates, 11-bit weights, truncating shifts
GRAY_BOUND = 0.503 + 1e-9  # _gray_cv4: exactly 0.503 over all 2^24 colours (15-bit weights, round half up)
REMAP_BOUND = 0.5 + 1e-9  # _remap_linear_u8 at the quantised coordinates: the 5-bit weights are exact, one rounding
# The chain resize -> gray -> remap: the float64 gray and remap are convex combinations (weights >= 0 summing to <= 1), so an input
# error passes through them no larger; each stage adds at most its own bound.  Resize + gray + remap < 1 + 0.503 + 0.5 = 2.003.


def chain_bound(resize, colour, remap):
    return (RESIZE_BOUND if resize else 0.0) + (GRAY_BOUND if colour else 0.0) + (REMAP_BOUND if remap else 0.0)


@pytest.fixture(scope="module")
def rigmod():
    util.pkg("build").build()
    return util.pkg("rig")


# ---------------------------------------------------------------------------------------------------------------- float64

def _resize_f64(src, dw, dh):
    """Bilinear resize [h,w,C] in float64 on OpenCV's coordinate map (d + 0.5) * (src / dst) - 0.5: columns clamp to the edge with
    weight 0, row indices are clipped.  Exact 2x in both axes is the mean of each 2x2 block."""
    sh, sw = src.shape[:2]
    S = src.astype(np.float64)
    if sw == 2 * dw and sh == 2 * dh:
        return (S[0::2, 0::2] + S[0::2, 1::2] + S[1::2, 0::2] + S[1::2, 1::2]) / 4

    def axis(n_dst, n_src):
        f = (np.arange(n_dst) + 0.5) * (n_src / n_dst) - 0.5
        i = np.floor(f).astype(np.int64)
        return i, f - i

    sx, fx = axis(dw, sw)
    edge = (sx < 0) | (sx >= sw - 1)
    fx = np.where(edge, 0.0, fx)
    sx = np.clip(sx, 0, sw - 1)
    sx1 = np.minimum(sx + 1, sw - 1)
    sy, fy = axis(dh, sh)
    y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    fx, fy = fx[None, :, None], fy[:, None, None]
    top = S[y0][:, sx] * (1 - fx) + S[y0][:, sx1] * fx
    bot = S[y1][:, sx] * (1 - fx) + S[y1][:, sx1] * fx
    return top * (1 - fy) + bot * fy


def _gray_f64(rgb):
    x = rgb.astype(np.float64)
    return 0.299 * x[..., 0] + 0.587 * x[..., 1] + 0.114 * x[..., 2]


def _remap_f64(img, mapx, mapy):
    """Bilinear remap in float64 at the quantised coordinates rint(map * 32) / 32; taps outside the source read 0."""
    H, W = img.shape
    qx, qy = np.rint(mapx.astype(np.float64) * 32) / 32, np.rint(mapy.astype(np.float64) * 32) / 32
    x0, y0 = np.floor(qx).astype(np.int64), np.floor(qy).astype(np.int64)
    fx, fy = qx - x0, qy - y0
    src = img.astype(np.float64)

    def at(x, y):
        ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        return np.where(ok, src[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)], 0.0)

    return (at(x0, y0) * (1 - fx) * (1 - fy) + at(x0 + 1, y0) * fx * (1 - fy) + at(x0, y0 + 1) * (1 - fx) * fy +
            at(x0 + 1, y0 + 1) * fx * fy)


def _chain_f64(rgb, fmt, W, H, maps_xy):
    """_expected_gray's chain in float64: resize (per channel) -> gray -> remap, no rounding anywhere."""
    x = rgb.astype(np.float64) if fmt != "gray" else _gray_cv4(rgb)[..., None].astype(np.float64)
    if x.shape[:2] != (H, W):
        x = _resize_f64(x, W, H)
    g = _gray_f64(x) if fmt != "gray" else x[..., 0]
    return _remap_f64(g, *maps_xy) if maps_xy is not None else g


def _random_maps(rng, W, H, sw, sh):
    """float32 maps over [-2, sw + 1] x [-2, sh + 1]: plenty of taps outside, some pixels with all four outside."""
    return (rng.uniform(-2, sw + 1, (H, W)).astype(np.float32), rng.uniform(-2, sh + 1, (H, W)).astype(np.float32))


# (src w, src h) -> (dst w, dst h): large non-integer downscale, exact 2x (the INTER_AREA shortcut), 2x in x only, near 2x,
# upscales, tiny sources
_RESIZE_PAIRS = [((1242, 375), (35, 33)), ((262, 134), (131, 67)), ((262, 67), (131, 67)), ((263, 135), (131, 67)), ((100, 50), (131, 67)),
                 ((50, 40), (123, 97)), ((2, 2), (32, 32)), ((1, 40), (32, 32)), ((2049, 70), (4099, 35))]


def test_resize_restatement_within_float64_bound():
    rng = np.random.default_rng(1)
    for (sw, sh), (dw, dh) in _RESIZE_PAIRS:
        src = rng.integers(0, 256, (sh, sw, 4), dtype=np.uint8)
        err = np.abs(_resize_linear_8uc4(src, dw, dh).astype(np.float64) - _resize_f64(src, dw, dh)).max()
        assert err < RESIZE_BOUND, ((sw, sh), (dw, dh), err)
    # a constant image stays constant (255 too: the alpha of 3-channel and gray sources)
    for v in (0, 255):
        assert (_resize_linear_8uc4(np.full((135, 263, 4), v, np.uint8), 131, 67) == v).all()


def test_gray_restatement_within_float64_bound():
    rgb = np.random.default_rng(2).integers(0, 256, (512, 512, 3), dtype=np.uint8)
    err = np.abs(_gray_cv4(rgb).astype(np.float64) - _gray_f64(rgb))
    assert err.max() <= GRAY_BOUND and err.max() > 0.49
    ends = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)
    assert _gray_cv4(ends).tolist() == [[0, 255, 76, 150, 29]]


def test_remap_restatement_within_float64_bound():
    rng = np.random.default_rng(3)
    for W, H in ((131, 67), (35, 33), (32, 32)):
        img = rng.integers(0, 256, (H, W), dtype=np.uint8)
        mx, my = _random_maps(rng, W, H, W, H)
        got = _remap_linear_u8(img, mx, my)
        err = np.abs(got.astype(np.float64) - _remap_f64(img, mx, my))
        assert err.max() <= REMAP_BOUND, (W, H, err.max())
        outside = (mx < -1) | (mx >= W) | (my < -1) | (my >= H)
        assert outside.sum() > 50 and (got[outside] == 0).all()  # every tap of these pixels is outside
    # integral coordinates: an exact copy
    jj, ii = np.meshgrid(np.arange(40, dtype=np.float32), np.arange(30, dtype=np.float32))
    img = rng.integers(0, 256, (30, 40), dtype=np.uint8)
    assert np.array_equal(_remap_linear_u8(img, jj, ii), img)


def test_chain_restatement_within_float64_bound():
    """_expected_gray (resize -> gray -> remap, as the kernels compute it) within chain_bound of the float64 chain."""
    rng = np.random.default_rng(4)
    for (sw, sh), (W, H) in _RESIZE_PAIRS[1:] + [((131, 67), (131, 67))]:
        rgb = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        for fmt in ("bgr", "gray"):
            for maps in (None, _random_maps(rng, W, H, W, H)):
                got = _expected_gray(rgb, fmt, W, H, maps).astype(np.float64)
                bound = chain_bound((sw, sh) != (W, H), fmt != "gray", maps is not None)
                err = np.abs(got - _chain_f64(rgb, fmt, W, H, maps)).max()
                assert err <= bound, ((sw, sh), (W, H), fmt, maps is not None, err, bound)


# ---------------------------------------------------------------------------------------------------------------- C ABI on the CPU

def test_frontend_device_argument_checks(rigmod):
    """sv_rig_frontend_device rejects these before it touches a device (no device is needed); batch = 0 is a no-op."""
    rc, r, L = _create(rigmod, _yaml(), 131, 67)
    assert rc == 0
    P = 4096  # any non-NULL, 4-byte aligned address: nothing is dereferenced on these paths
    try:
        def call(batch=1, sw=131, sh=67, pitch=None, fmt=0, left=P, right=P, gl=P, gr=P, col=None):
            pitch = sw * _CH[FORMATS[fmt]] if pitch is None else pitch
            return L.sv_rig_frontend_device(r, left, right, batch, sw, sh, pitch, fmt, gl, gr, col, None)

        # W = 131, H = 67: 33 groups per row, 9 tiles of 256 lanes, 18 blocks per pair: 2^31 // 18 + 1 pairs do not fit a launch
        bad = [(dict(batch=-1), "batch"), (dict(left=None), "NULL"), (dict(right=None), "NULL"), (dict(gl=None), "NULL"), (dict(gr=None), "NULL"),
               (dict(col=P + 1), "aligned"), (dict(col=P + 2), "aligned"), (dict(batch=2 ** 31 // 18 + 1), "too large"),
               (dict(batch=2 ** 31 - 1), "too large"), (dict(sw=8193, sh=8192, pitch=4 * 8193), "2^26"), (dict(sw=8192, sh=8193, pitch=4 * 8192), "2^26")]
        for fmt, c in enumerate((4, 3, 3, 1)):
            bad.append((dict(fmt=fmt, pitch=131 * c - 1), "pitch"))
            bad.append((dict(fmt=fmt, sw=1, sh=1, pitch=c - 1), "pitch"))
        for kw, word in bad:
            assert call(**kw) == SV_ERR_ARG, kw
            assert word in L.sv_rig_last_error(r).decode(), (kw, L.sv_rig_last_error(r))
        assert call(batch=0) == SV_OK
        assert call(batch=0, sw=8192, sh=8192, pitch=4 * 8192) == SV_OK  # exactly 2^26 pixels passes the size check
        assert call(batch=0, sw=8192, sh=8192, pitch=8192, fmt=3) == SV_OK
        assert call(batch=0, sw=1, sh=1, pitch=3, fmt=1) == SV_OK
    finally:
        L.sv_rig_destroy(r)


def _border_counts(m, W, H):
    """Per side: pixels with a nonzero-weight remap tap outside the W x H source, and pixels whose four taps are all outside."""
    out = []
    for s in (0, 1):
        sx, sy = np.rint(m[2 * s] * np.float32(32)).astype(np.int64), np.rint(m[2 * s + 1] * np.float32(32)).astype(np.int64)
        ix, iy, fx, fy = sx >> 5, sy >> 5, sx & 31, sy & 31
        taps = [(ix, iy, np.ones(ix.shape, bool)), (ix + 1, iy, fx > 0), (ix, iy + 1, fy > 0), (ix + 1, iy + 1, (fx > 0) & (fy > 0))]
        some, every = np.zeros(ix.shape, bool), np.ones(ix.shape, bool)
        for x, y, w in taps:
            o = (x < 0) | (x >= W) | (y < 0) | (y >= H)
            some |= o & w
            every &= o
        out.append((int(some.sum()), int(every.sum())))
    return out


# synthetic calibrations whose maps leave the image: (W, H, K, T, D, scale, pixels with a tap outside, pixels all outside) per side
def _border_calibrations():
    W2, H2, s = 333, 101, 0.5
    return {"edge": (131, 67, [[120, 0, 66], [0, 118, 33], [0, 0, 1]], (-0.5, 0, 0), None, 0.5, 134, 67),
            "partial": (W2, H2, [[120, 0, W2 * s / 2], [0, 118, H2 * s / 2], [0, 0, 1]], (-0.3, 0, 0.3), (-0.3, 0.1, 0, 0, 0), s, 4747, 0)}


def _border_rig(rigmod, tmp_path, name):
    W, H, K, T, D, scale, n_some, n_all = _border_calibrations()[name]
    path = _write_calibration(tmp_path / (name + ".yml"), np.array(K, np.float64), np.array(T, np.float64), D=None if D is None else np.array(D, np.float64))
    return rigmod.StereoRig(W, H, calibration=path, rectify=True, scale=scale), n_some, n_all


@pytest.mark.parametrize("name", ["edge", "partial"])
def test_border_calibrations_reach_outside(rigmod, tmp_path, name):
    """The maps of the synthetic calibrations put remap taps outside the source (lower bounds: if map generation changes and the
    border coverage disappears, this fails)."""
    rig, n_some, n_all = _border_rig(rigmod, tmp_path, name)
    try:
        m = rig.maps()
        for some, every in _border_counts(m, rig.width, rig.height):
            assert some >= n_some and every >= n_all, (name, some, every)
    finally:
        rig.close()


# ---------------------------------------------------------------------------------------------------------------- GPU

def _frames(B, sh, sw, seed):
    """B RGB frames [B,sh,sw,3]: the colour KITTI fixture tiled from a seeded origin with seeded per-channel offsets (mod 256), a
    quarter of the pixels replaced by seeded noise."""
    base = util.load_png("kitti0_color_left.png")
    rng = np.random.default_rng(seed)
    y0, x0 = rng.integers(0, base.shape[0]), rng.integers(0, base.shape[1])
    tile = base[(y0 + np.arange(sh)) % base.shape[0]][:, (x0 + np.arange(sw)) % base.shape[1]].astype(np.int64)
    out = np.empty((B, sh, sw, 3), np.uint8)
    for b in range(B):
        f = (tile + rng.integers(0, 256, 3)) % 256
        mask = rng.random((sh, sw)) < 0.25
        f[mask] = rng.integers(0, 256, (int(mask.sum()), 3))
        out[b] = f
    return out


# source layouts: (row padding in bytes, byte offset of the first frame in its buffer)
LAYOUTS = {"pad0": (0, 0), "pad1": (1, 0), "pad3": (3, 0), "odd": (0, 1)}


def _device(a, pad, offset):
    """Frames [B,h,w(,C)] as a CUDA view with rows w*C + pad bytes apart, starting `offset` bytes into a buffer sized exactly."""
    import torch
    B, h, w = a.shape[:3]
    C = a.shape[3] if a.ndim == 4 else 1
    pitch = w * C + pad
    host = np.full((offset + B * h * pitch,), 77, np.uint8)
    rows = host[offset:].reshape(B, h, pitch)
    rows[:, :, :w * C] = a.reshape(B, h, w * C)
    buf = torch.from_numpy(host).cuda()
    size, stride = ((B, h, w, C), (h * pitch, pitch, C, 1)) if a.ndim == 4 else ((B, h, w), (h * pitch, pitch, 1))
    v = torch.as_strided(buf, size, stride, offset)
    assert v.data_ptr() % 2 == offset % 2 and v.stride(1) == pitch
    return v


def _bgra_of(src, fmt):
    """A source in `fmt` as the kernels expand each pixel: B, G, R, A (A = 255 for 3-channel and gray sources)."""
    if fmt == "bgra":
        return src
    a = np.full((src.shape if fmt == "gray" else src.shape[:-1]) + (1,), 255, np.uint8)
    if fmt == "bgr":
        return np.concatenate([src, a], -1)
    if fmt == "rgb":
        return np.concatenate([src[..., ::-1], a], -1)
    return np.concatenate([np.repeat(src[..., None], 3, -1), a], -1)


def _check_frontend(rig, rgb_l, rgb_r, fmt, layout, label):
    """Runs the rig's front end on the pair in `fmt` and `layout` with colours; asserts gray == the restatement, gray within the
    chain bound of float64, and the colours of every pair b."""
    W, H = rig.width, rig.height
    B, sh, sw = rgb_l.shape[:3]
    resize = (sw, sh) != (W, H)
    maps = rig.maps()
    L, R = _as_format(rgb_l, fmt, 1), _as_format(rgb_r, fmt, 2)
    pad, off = LAYOUTS[layout]
    gl, gr, col = (t.cpu().numpy() for t in rig.frontend(_device(L, pad, off), _device(R, pad, off), pixel_format=fmt, colors=True))
    assert gl.shape == gr.shape == (B, H, W) and col.shape == (B, H, W, 4)
    bound = chain_bound(resize, fmt != "gray", maps is not None)
    for b in range(B):
        for s, rgb, got in ((0, rgb_l, gl), (1, rgb_r, gr)):
            mxy = (maps[2 * s], maps[2 * s + 1]) if maps is not None else None
            want = _expected_gray(rgb[b], fmt, W, H, mxy)
            assert np.array_equal(got[b], want), (label, "side", s, "pair", b, int((got[b] != want).sum()))
            err = np.abs(got[b].astype(np.float64) - _chain_f64(rgb[b], fmt, W, H, mxy)).max()
            assert err <= bound, (label, "side", s, "pair", b, err, bound)
        want_c = _bgra_of(L[b], fmt)  # unrectified: k_rig_direct writes the source pixels, the resize pass the resized ones
        if resize:
            want_c = _resize_linear_8uc4(want_c, W, H)
        assert np.array_equal(col[b], want_c), (label, "colours of pair", b, int((col[b] != want_c).any(-1).sum()))
    return gl, gr


# (rig, source): same size with W % 4 == 3 (direct pass and fused remap) ...
_SAME = [((131, 67), (131, 67))]
# ... and through the resize pass (with rectification: then the remap pass)
_RESIZED = [((35, 33), (1242, 375)),  # large non-integer downscale
            ((131, 67), (262, 134)),  # exact 2x: the INTER_AREA shortcut
            ((131, 67), (262, 67)),  # 2x in x only: the linear path
            ((131, 67), (263, 135)),  # near 2x
            ((131, 67), (100, 50)),  # non-integer upscale
            ((32, 32), (1, 1)), ((32, 32), (1, 40)), ((32, 32), (40, 1)), ((32, 32), (2, 2)),  # smallest rig, tiny sources
            ((2484, 750), (1242, 375)),  # exact 2x upscale
            ((4099, 35), (2049, 70))]  # wide, W % 4 == 3: upscale in x, downscale in y


def _matrix():
    """Every (pass, format) meets every geometry of its pass and every source layout at least once; B alternates 1 / 5 (B = 1 on
    the two large rigs)."""
    lay = list(LAYOUTS)
    cases = []
    for p, (rectify, geoms) in enumerate(((False, _SAME), (True, _SAME), (False, _RESIZED), (True, _RESIZED))):
        for f, fmt in enumerate(FORMATS):
            todo = [(g, lay[(i + f + p) % 4]) for i, g in enumerate(geoms)]
            while len(todo) < len(lay):  # one geometry: repeat it for the remaining layouts
                todo.append((geoms[0], lay[(len(todo) + f + p) % 4]))
            for i, ((rig, src), layout) in enumerate(todo):
                B = 1 if rig[0] * rig[1] > 100000 or (i + f) % 2 else 5
                cases.append(pytest.param(rig, src, fmt, layout, rectify, B,
                                          id="%dx%d-from-%dx%d-%s-%s-%s-B%d" % (rig + src + (fmt, layout, "rect" if rectify else "plain", B))))
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("rig_size,src_size,fmt,layout,rectify,B", _matrix())
def test_frontend_edges(rigmod, rig_size, src_size, fmt, layout, rectify, B):
    (W, H), (sw, sh) = rig_size, src_size
    seed = zlib.crc32(("%s %s %s %s %d %d" % (rig_size, src_size, fmt, layout, rectify, B)).encode())
    rgb_l, rgb_r = _frames(B, sh, sw, seed), _frames(B, sh, sw, seed + 1)
    rig = rigmod.StereoRig(W, H, rectify=rectify, scale=1242 / W)
    try:
        if rectify:  # the KITTI maps, scaled to the rig, mostly stay inside the image: the remapped gray is not all border
            m = rig.maps()
            inside = (m[0] >= 0) & (m[0] <= W - 1) & (m[1] >= 0) & (m[1] <= H - 1)
            assert inside.mean() > 0.5
        _check_frontend(rig, rgb_l, rgb_r, fmt, layout, (rig_size, src_size, fmt, layout, rectify, B))
    finally:
        rig.close()


@pytest.mark.gpu
@pytest.mark.parametrize("resize", [False, True])
@pytest.mark.parametrize("name", ["edge", "partial"])
def test_remap_borders(rigmod, tmp_path, name, resize):
    """Synthetic calibrations whose remap taps leave the source (BORDER_CONSTANT): fused direct + remap pass without resize, resize
    then remap pass with it; every format, B = 2."""
    rig, n_some, n_all = _border_rig(rigmod, tmp_path, name)
    try:
        W, H = rig.width, rig.height
        for some, every in _border_counts(rig.maps(), W, H):
            assert some >= n_some and every >= n_all
        sw, sh = (W * 3 // 2 + 1, H * 3 // 2) if resize else (W, H)
        for f, fmt in enumerate(FORMATS):
            seed = zlib.crc32(("%s %d %s" % (name, resize, fmt)).encode())
            _check_frontend(rig, _frames(2, sh, sw, seed), _frames(2, sh, sw, seed + 1), fmt, list(LAYOUTS)[f], (name, resize, fmt))
    finally:
        rig.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [65, 66, 131])  # W % 4 == 1, 2, 3
def test_writes_stay_inside_the_outputs(rigmod, W):
    """sv_rig_frontend_device called directly with the grays at byte offsets 1 and 2 from a 4-byte boundary and the colours at a
    4-byte, not 16-byte, offset inside sentinel-filled buffers: nothing outside B*H*W (gray) and 4*B*H*W (colour) bytes changes, and
    the values inside are rig.frontend's.  Rejected calls and batch = 0 change nothing at all."""
    import torch
    H, B, G, SENT = 37, 2, 64, 0xA5
    N = B * H * W
    L = rigmod.rig_lib()
    st = torch.cuda.current_stream().cuda_stream
    for rectify in (False, True):
        rig = rigmod.StereoRig(W, H, rectify=rectify, scale=1242 / W)
        try:
            for resize in (False, True):
                fmt = FORMATS[(W + 2 * rectify + resize) % 4]
                sw, sh = (W * 3 // 2 + 1, H * 3 // 2 + 1) if resize else (W, H)
                seed = zlib.crc32(("%d %d %d" % (W, rectify, resize)).encode())
                l, r = _as_format(_frames(B, sh, sw, seed), fmt, 1), _as_format(_frames(B, sh, sw, seed + 1), fmt, 2)
                dl, dr = torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()
                pitch = sw * _CH[fmt]
                want_l, want_r, want_c = (t.cpu().numpy() for t in rig.frontend(dl, dr, pixel_format=fmt, colors=True))

                def buffers():
                    return tuple(torch.full((2 * G + n,), SENT, dtype=torch.uint8, device="cuda") for n in (N, N, 4 * N))

                def run(bufs, batch=B, pitch=pitch, fmt=fmt, left=dl.data_ptr(), col_off=G + 4):
                    bl, br, bc = bufs
                    return L.sv_rig_frontend_device(rig._h, left, dr.data_ptr(), batch, sw, sh, pitch, _FMT[fmt], bl.data_ptr() + G + 1,
                                                    br.data_ptr() + G + 2, bc.data_ptr() + col_off, st)

                bufs = buffers()
                assert all(b.data_ptr() % 16 == 0 for b in bufs)
                assert run(bufs) == SV_OK
                torch.cuda.synchronize()
                bl, br, bc = (b.cpu().numpy() for b in bufs)
                label = (W, rectify, resize, fmt)
                for buf, start, n in ((bl, G + 1, N), (br, G + 2, N), (bc, G + 4, 4 * N)):
                    assert (buf[:start] == SENT).all() and (buf[start + n:] == SENT).all(), label
                assert np.array_equal(bl[G + 1:G + 1 + N], want_l.reshape(-1)), label
                assert np.array_equal(br[G + 2:G + 2 + N], want_r.reshape(-1)), label
                assert np.array_equal(bc[G + 4:G + 4 + 4 * N], want_c.reshape(-1)), label

                bufs = buffers()
                rejected = [run(bufs, col_off=G + 5), run(bufs, col_off=G + 6), run(bufs, pitch=pitch - 1), run(bufs, batch=-1),
                            run(bufs, left=None), run(bufs, batch=2 ** 31 - 1), run(bufs, fmt="bgra", pitch=4 * sw - 1)]
                assert rejected == [SV_ERR_ARG] * len(rejected), label
                assert run(bufs, batch=0) == SV_OK
                torch.cuda.synchronize()
                assert all(bool((b == SENT).all().item()) for b in bufs), label
        finally:
            rig.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(131, 67), (35, 33)])
def test_chain_at_odd_rig_sizes(rigmod, oracle, W, H):
    """The colour KITTI pair resized to a small rig and rectified, through point_clouds(colors=True) and top_view ("dmap" and "d1"):
    d1 == the oracle on the restatement's grays, dmap / points == the float64 reprojection, grids == points_2_top_view of them."""
    sv = util.pkg("stereo_vision.sv")
    rgb_l, rgb_r = util.load_png("kitti0_color_left.png"), util.load_png("kitti0_color_right.png")
    bgr_l, bgr_r = np.ascontiguousarray(rgb_l[..., ::-1]), np.ascontiguousarray(rgb_r[..., ::-1])
    dmap_grid = dict(x_range=(-10, 10), y_range=(-4, 4), z_range=(0, 30), scale=8)  # quarter-depth clouds, camera axes
    d1_grid = dict(sv.CLI_TOP_VIEW)
    xf = (sv.CAMERA_TO_VEHICLE, None)
    rig = rigmod.StereoRig(W, H, rectify=True, scale=1242 / W)
    try:
        maps, Q = rig.maps(), rig.Q.copy()
        d1, dmap, pts, col = rig.point_clouds(bgr_l, bgr_r, pixel_format="bgr", colors=True)
        g_dmap = rig.top_view(bgr_l, bgr_r, pixel_format="bgr", disparity="dmap", **dmap_grid)
        g_d1 = rig.top_view(bgr_l, bgr_r, pixel_format="bgr", disparity="d1", transform=xf, **d1_grid)
    finally:
        rig.close()
    gl = _expected_gray(rgb_l, "bgr", W, H, (maps[0], maps[1]))
    gr = _expected_gray(rgb_r, "bgr", W, H, (maps[2], maps[3]))
    o1, _, _ = oracle.process(ElasParams.driver(255), gl, gr)
    assert (o1 > 0).sum() > W * H // 10
    assert np.array_equal(d1[0].view(np.uint32), o1.view(np.uint32))
    assert np.array_equal(dmap[0], np.clip(np.rint(o1 * np.float32(4.0)), 0, 255).astype(np.uint8))
    want_pts = _reproject_np(o1[None], Q)
    assert np.array_equal(pts, want_pts, equal_nan=True)
    assert np.array_equal(col[0], _resize_linear_8uc4(_bgra_of(bgr_l[None], "bgr")[0], W, H))
    want_dmap = sv.points_2_top_view(want_pts[0].reshape(-1, 3), **dmap_grid)
    want_d1 = sv.points_2_top_view(_d1_points(o1[None], Q, *xf)[0], **d1_grid)
    assert (want_dmap > 0).any() and (want_d1 > 0).any()
    assert np.array_equal(g_dmap[0], want_dmap) and np.array_equal(g_d1[0], want_d1)
