"""TEST INFRASTRUCTURE — ctypes front-end for the two CPU checkers.

* ``Oracle``  : our CPU restatement (oracle/liboracle.so, built from oracle/elas_oracle.cpp)
* ``RefElas`` : the reference's own serial LIBELAS (oracle/_ref/libelas_ref.so, built in the
                container from /root/reference by oracle/Makefile; may be absent elsewhere)

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


class ElasParams(ctypes.Structure):
    """Mirror of oracle/elas_params.h (== Elas::parameters, reference elas.h:60-145)."""

    _fields_ = [
        ("disp_min", ctypes.c_int32),
        ("disp_max", ctypes.c_int32),
        ("support_threshold", ctypes.c_float),
        ("support_texture", ctypes.c_int32),
        ("candidate_stepsize", ctypes.c_int32),
        ("incon_window_size", ctypes.c_int32),
        ("incon_threshold", ctypes.c_int32),
        ("incon_min_support", ctypes.c_int32),
        ("add_corners", ctypes.c_int32),
        ("grid_size", ctypes.c_int32),
        ("beta", ctypes.c_float),
        ("gamma", ctypes.c_float),
        ("sigma", ctypes.c_float),
        ("sradius", ctypes.c_float),
        ("match_texture", ctypes.c_int32),
        ("lr_threshold", ctypes.c_int32),
        ("speckle_sim_threshold", ctypes.c_float),
        ("speckle_size", ctypes.c_int32),
        ("ipol_gap_width", ctypes.c_int32),
        ("filter_median", ctypes.c_int32),
        ("filter_adaptive_mean", ctypes.c_int32),
        ("postprocess_only_left", ctypes.c_int32),
        ("subsampling", ctypes.c_int32),
    ]

    @classmethod
    def preset(cls, setting):
        """setting: 'robotics' | 'middlebury' (elas.h:92-143)."""
        p = cls()
        p.disp_min, p.disp_max = 0, 255
        p.support_texture, p.candidate_stepsize = 10, 5
        p.incon_window_size, p.incon_threshold, p.incon_min_support = 5, 5, 5
        p.grid_size, p.beta, p.sigma = 20, 0.02, 1.0
        p.lr_threshold, p.speckle_sim_threshold, p.speckle_size = 2, 1.0, 200
        p.subsampling = 0
        if setting == "robotics":
            p.support_threshold, p.add_corners, p.gamma, p.sradius = 0.85, 0, 3.0, 2.0
            p.match_texture, p.ipol_gap_width = 1, 3
            p.filter_median, p.filter_adaptive_mean, p.postprocess_only_left = 0, 1, 1
        elif setting == "middlebury":
            p.support_threshold, p.add_corners, p.gamma, p.sradius = 0.95, 1, 5.0, 3.0
            p.match_texture, p.ipol_gap_width = 0, 5000
            p.filter_median, p.filter_adaptive_mean, p.postprocess_only_left = 1, 0, 0
        else:
            raise ValueError(setting)
        return p

    @classmethod
    def driver(cls, disp_max=255):
        """What the reference driver runs (stereo_vision.cpp:307-311)."""
        p = cls.preset("middlebury")
        p.postprocess_only_left = 1
        p.filter_adaptive_mean = 1
        p.disp_max = disp_max
        return p


_STAGE_DTYPES = {
    "desc1": np.uint8, "desc2": np.uint8,
    "dcan_raw": np.int16, "dcan_dims": np.int32,
    "support": np.int32, "tri1": np.int32, "tri2": np.int32,
    "planes1": np.float32, "planes2": np.float32,
    "grid1": np.int32, "grid2": np.int32, "grid_dims": np.int32, "tri_id1": np.int32, "tri_id2": np.int32,
}


def _stage_dtype(name):
    return _STAGE_DTYPES.get(name, np.float32)


def _u8(a):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


class _StageLib:
    """Common `*_run_stages / *_size / *_get` protocol."""

    prefix = None

    def __init__(self, path):
        self.path = path
        self.lib = ctypes.CDLL(path)
        L, pf = self.lib, self.prefix
        self._run = getattr(L, pf + "_run_stages")
        self._run.restype = ctypes.c_int
        self._run.argtypes = [ctypes.POINTER(ElasParams), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8),
                              ctypes.c_int, ctypes.c_int, ctypes.c_int]
        self._size = getattr(L, pf + "_size")
        self._size.restype = ctypes.c_long
        self._size.argtypes = [ctypes.c_char_p]
        self._get = getattr(L, pf + "_get")
        self._get.restype = ctypes.c_long
        self._get.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_long]
        self._proc = getattr(L, pf + "_process")
        self._proc.restype = ctypes.c_double
        self._proc.argtypes = [ctypes.POINTER(ElasParams), ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8),
                               ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                               ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_int]
        self._delaunay = getattr(L, pf + "_delaunay")
        self._delaunay.restype = ctypes.c_int
        self._delaunay.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]

    def run_stages(self, params, left, right):
        """Run the whole pipeline keeping every intermediate; returns #support points."""
        H, W = left.shape
        l, lp = _u8(left)
        r, rp = _u8(right)
        n = self._run(ctypes.byref(params), lp, rp, W, H, W)
        if n < 0:
            raise RuntimeError("%s_run_stages failed: %d" % (self.prefix, n))
        return n

    def stage(self, name, shape=None):
        n = self._size(name.encode())
        if n < 0:
            raise KeyError(name)
        dt = np.dtype(_stage_dtype(name))
        out = np.empty(n // dt.itemsize, dtype=dt)
        got = self._get(name.encode(), out.ctypes.data_as(ctypes.c_void_p), n)
        assert got == n
        return out.reshape(shape) if shape is not None else out

    def stages(self, names):
        return {k: self.stage(k) for k in names}

    def process(self, params, left, right, canonical=True, reps=1):
        """Operator-seam call (Elas::process semantics).  Returns (D1, D2, seconds_per_call)."""
        H, W = left.shape
        l, lp = _u8(left)
        r, rp = _u8(right)
        Hm, Wm = (H // 2, W // 2) if params.subsampling else (H, W)  # elas.h:160-161: half-size maps when subsampling
        D1 = np.zeros((Hm, Wm), np.float32)
        D2 = np.zeros((Hm, Wm), np.float32)
        t = self._proc(ctypes.byref(params), lp, rp, W, H, W, D1.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                       D2.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(bool(canonical)), int(reps))
        return D1, D2, t

    def delaunay(self, xy):
        """xy: (n,2) float32 points -> (nt,3) int32 triangles in the reference's output order."""
        xy = np.ascontiguousarray(xy, dtype=np.float32)
        n = xy.shape[0]
        cap = 2 * n + 16
        out = np.empty((cap, 3), np.int32)
        nt = self._delaunay(xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cap)
        assert 0 <= nt <= cap
        return out[:nt].copy()


class RefElas(_StageLib):
    prefix = "ref"
    default_path = os.path.join(HERE, "_ref", "libelas_ref.so")

    @classmethod
    def available(cls):
        return os.path.exists(cls.default_path)

    def __init__(self, path=None):
        super().__init__(path or self.default_path)


class Oracle(_StageLib):
    prefix = "orc"
    default_path = os.path.join(HERE, "liboracle.so")

    def __init__(self, path=None):
        path = path or self.default_path
        if not os.path.exists(path):
            build()
        super().__init__(path)
        fp, pp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ElasParams)
        for name, args in (("orc_lr_check", [pp, fp, fp]), ("orc_speckle", [pp, fp]), ("orc_gap", [pp, fp]),
                           ("orc_adaptive_mean", [fp]), ("orc_adaptive_mean_sub", [fp]), ("orc_median", [fp])):
            f = getattr(self.lib, name)
            f.restype = None
            f.argtypes = args + [ctypes.c_int, ctypes.c_int]

        ip, vp = ctypes.c_int, ctypes.c_void_p
        for name, res, args in (("orc_descriptor", None, [vp, ip, ip, ip, vp]), ("orc_support_filter", ip, [pp, vp, ip, ip, vp, ip]),
                                ("orc_planes", None, [vp, vp, ip, vp]), ("orc_grid", None, [pp, vp, ip, ip, ip, ip, vp]),
                                ("orc_raster", None, [vp, vp, ip, ip, ip, ip, vp]), ("orc_dense", None, [pp, vp, vp, vp, ip, vp, vp, vp, ip, ip, ip, vp])):
            f = getattr(self.lib, name)
            f.restype, f.argtypes = res, args

    # ---- the stages between the support lattice and the dense maps, on a support list of the caller's choice
    @staticmethod
    def grid_dims(params, W, H):
        """(disp_max + 2, cells per row, cell rows): elas.cpp:88-90 (ceil of a float division)."""
        f = np.float32
        return params.disp_max + 2, int(np.ceil(f(W) / f(params.grid_size))), int(np.ceil(f(H) / f(params.grid_size)))

    def descriptor(self, params, image):
        """uint8 [H, W, 16]; at half resolution only the rows 4, 6, .. < H - 3 are filled (descriptor.cpp:48-93), as the pipeline does."""
        img, _ = _u8(image)
        H, W = img.shape
        desc = np.zeros((H, W, 16), np.uint8)
        self.lib.orc_descriptor(img.ctypes.data, W, H, W, desc.ctypes.data)
        if params.subsampling:
            desc[:4] = 0
            desc[1::2] = 0
        return desc

    def support_filter(self, params, lattice, W, H):
        """int16 [Hc, Wc] lattice (left unchanged) -> int32 [n, 3] support list (u, v, d)."""
        lat = np.array(lattice, np.int16, order="C")
        out = np.zeros((lat.size + 6, 3), np.int32)
        n = self.lib.orc_support_filter(ctypes.byref(params), lat.ctypes.data, W, H, out.ctypes.data, out.shape[0])
        assert 0 <= n <= out.shape[0]
        return out[:n].copy()

    def planes(self, support, tri):
        """float32 [nt, 6]: t1a t1b t1c t2a t2b t2c per triangle."""
        support, tri = np.ascontiguousarray(support, np.int32), np.ascontiguousarray(tri, np.int32)
        out = np.zeros((len(tri), 6), np.float32)
        self.lib.orc_planes(support.ctypes.data, tri.ctypes.data, len(tri), out.ctypes.data)
        return out

    def grid(self, params, support, W, H, right_image):
        """int32 [cell rows, cells per row, disp_max + 2]: count, then the cell's candidate disparities in ascending order."""
        support = np.ascontiguousarray(support, np.int32)
        gd = self.grid_dims(params, W, H)
        out = np.zeros((gd[2], gd[1], gd[0]), np.int32)
        self.lib.orc_grid(ctypes.byref(params), support.ctypes.data, len(support), W, H, int(bool(right_image)), out.ctypes.data)
        return out

    def raster(self, support, tri, W, H, right_image):
        """int32 [H, W]: the last triangle in list order whose scan conversion covers the pixel, -1 for none (full resolution)."""
        support, tri = np.ascontiguousarray(support, np.int32), np.ascontiguousarray(tri, np.int32)
        out = np.zeros((H, W), np.int32)
        self.lib.orc_raster(support.ctypes.data, tri.ctypes.data, len(tri), W, H, int(bool(right_image)), out.ctypes.data)
        return out

    def dense(self, params, support, tri, planes, grid, desc1, desc2, right_image):
        """float32 winner-takes-all map, [H, W] or [H // 2, W // 2] at half resolution."""
        support, tri = np.ascontiguousarray(support, np.int32), np.ascontiguousarray(tri, np.int32)
        planes, grid = np.ascontiguousarray(planes, np.float32), np.ascontiguousarray(grid, np.int32)
        desc1, desc2 = np.ascontiguousarray(desc1, np.uint8), np.ascontiguousarray(desc2, np.uint8)
        H, W = desc1.shape[:2]
        out = np.zeros((H // 2, W // 2) if params.subsampling else (H, W), np.float32)
        self.lib.orc_dense(ctypes.byref(params), support.ctypes.data, tri.ctypes.data, planes.ctypes.data, len(tri), grid.ctypes.data, desc1.ctypes.data,
                           desc2.ctypes.data, W, H, int(bool(right_image)), out.ctypes.data)
        return out

    def chain_from_lattice(self, params, lattice, left, right):
        """Everything between a support lattice and the dense maps of an image pair, stage by stage: support, tri1/2, planes1/2, grid1/2,
        tri_id1/2, wta1/2 (the pipeline's names).  With fewer than three support points only the list."""
        H, W = left.shape
        sup = self.support_filter(params, lattice, W, H)
        out = {"support": sup}
        if len(sup) < 3:
            return out
        d1, d2 = self.descriptor(params, left), self.descriptor(params, right)
        for side, key in ((0, "1"), (1, "2")):
            xy = np.stack([sup[:, 0] - side * sup[:, 2], sup[:, 1]], 1)
            tri = self.delaunay(xy)
            pl = self.planes(sup, tri)
            g = self.grid(params, sup, W, H, side)
            out.update({"tri" + key: tri, "planes" + key: pl, "grid" + key: g, "tri_id" + key: self.raster(sup, tri, W, H, side),
                        "wta" + key: self.dense(params, sup, tri, pl, g, d1, d2, side)})
        return out

    # ---- the post-processing stages on maps of the caller's choice; each returns new float32 [H, W] maps, the arguments stay as they are
    @staticmethod
    def _map(D):
        D = np.array(D, dtype=np.float32, order="C")  # (a copy: the stages work in place)
        assert D.ndim == 2
        return D, D.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

    def lr_check(self, params, D1, D2):
        (D1, p1), (D2, p2) = self._map(D1), self._map(D2)
        assert D1.shape == D2.shape
        self.lib.orc_lr_check(ctypes.byref(params), p1, p2, D1.shape[1], D1.shape[0])
        return D1, D2

    def speckle(self, params, D):
        D, p = self._map(D)
        self.lib.orc_speckle(ctypes.byref(params), p, D.shape[1], D.shape[0])
        return D

    def gap(self, params, D):
        D, p = self._map(D)
        self.lib.orc_gap(ctypes.byref(params), p, D.shape[1], D.shape[0])
        return D

    def adaptive_mean(self, D, sub=False):
        """sub: the half-resolution branch (elas.cpp:1332-1397), what the pipeline takes with params.subsampling."""
        D, p = self._map(D)
        (self.lib.orc_adaptive_mean_sub if sub else self.lib.orc_adaptive_mean)(p, D.shape[1], D.shape[0])
        return D

    def median(self, D):
        D, p = self._map(D)
        self.lib.orc_median(p, D.shape[1], D.shape[0])
        return D


def build(ref=True):
    """Compile the checker(s).  Building the checker is not using it."""
    subprocess.check_call(["make", "-s", "-C", HERE, "liboracle.so"])
    if ref:
        subprocess.check_call(["make", "-s", "-C", HERE, "ref"])
