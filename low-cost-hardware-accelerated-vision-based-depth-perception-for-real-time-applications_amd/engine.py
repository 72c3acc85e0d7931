"""Python front-end of libstereo_vision_hip.so (ctypes over the C ABI of include/stereo_vision_hip.h).

PyTorch is used only as plumbing: device memory (tensors), the current device and torch.distributed in bench.py.
All compute is in the hand-written HIP kernels behind the C ABI; there is no eager/CPU fallback — if the
library is missing or no GPU is present, calls fail loudly.
"""
import ctypes
import os

import numpy as np

# The engine drives six HIP streams (two for the first GPU phase, four for the second) next to the application's own; ROCm
# maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and streams that share a queue serialise.  8 measured +2 %
# pairs/s over the default, 6 slightly less than the default.  Only effective before the process's first HIP call;
# an explicit setting of the application wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SV_LIB_PATH") or os.path.join(HERE, "libstereo_vision_hip.so")  # SV_LIB_PATH: kernel experiments only

SV_ROBOTICS, SV_MIDDLEBURY, SV_DRIVER = 0, 1, 2


class SvParams(ctypes.Structure):
    """sv_params == Elas::parameters (reference: src/serial_includes/elas/elas.h:60-145)."""

    _fields_ = [
        ("disp_min", ctypes.c_int32), ("disp_max", ctypes.c_int32), ("support_threshold", ctypes.c_float),
        ("support_texture", ctypes.c_int32), ("candidate_stepsize", ctypes.c_int32), ("incon_window_size", ctypes.c_int32),
        ("incon_threshold", ctypes.c_int32), ("incon_min_support", ctypes.c_int32), ("add_corners", ctypes.c_int32),
        ("grid_size", ctypes.c_int32), ("beta", ctypes.c_float), ("gamma", ctypes.c_float), ("sigma", ctypes.c_float),
        ("sradius", ctypes.c_float), ("match_texture", ctypes.c_int32), ("lr_threshold", ctypes.c_int32),
        ("speckle_sim_threshold", ctypes.c_float), ("speckle_size", ctypes.c_int32), ("ipol_gap_width", ctypes.c_int32),
        ("filter_median", ctypes.c_int32), ("filter_adaptive_mean", ctypes.c_int32), ("postprocess_only_left", ctypes.c_int32),
        ("subsampling", ctypes.c_int32),
    ]

    @classmethod
    def preset(cls, setting):
        p = cls()
        code = {"robotics": SV_ROBOTICS, "middlebury": SV_MIDDLEBURY, "driver": SV_DRIVER}[setting]
        lib().sv_params_init(ctypes.byref(p), code)
        return p

    @classmethod
    def driver(cls, disp_max=255):
        """MIDDLEBURY + postprocess_only_left + adaptive mean: what the reference driver runs (stereo_vision.cpp:307-311)."""
        p = cls.preset("driver")
        p.disp_max = disp_max
        return p


class SvConfig(ctypes.Structure):
    """sv_config of include/stereo_vision_hip.h: 0 = the default for every field."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("device", ctypes.c_int32), ("n_workers", ctypes.c_int32),
                ("chunk", ctypes.c_int32), ("keep_debug", ctypes.c_int32), ("n_streams", ctypes.c_int32), ("n_slots", ctypes.c_int32),
                ("gpu_lattice_filter", ctypes.c_int32), ("gpu_triangulation", ctypes.c_int32), ("gpu_triangulation_pct", ctypes.c_int32),
                ("resident", ctypes.c_int32), ("dg_sub_max", ctypes.c_int32), ("dg_max_points", ctypes.c_int32), ("affinity", ctypes.c_int32),
                ("inline_latency_path", ctypes.c_int32), ("event_sync", ctypes.c_int32), ("share_sliced", ctypes.c_int32), ("latency_split", ctypes.c_int32), ("host_copies", ctypes.c_int32), ("reserved", ctypes.c_int32 * 4)]


_TRIANGULATION_MODES = {None: 0, "auto": 0, "gpu": 1, "host": 2, "balanced": 4}


_lib = None

_STAGE_DTYPES = {"desc1": np.uint8, "desc2": np.uint8, "dcan_raw": np.int16, "dcan_dims": np.int32, "support": np.int32,
                 "tri1": np.int32, "tri2": np.int32, "grid1": np.int32, "grid2": np.int32, "grid_dims": np.int32,
                 "tri_id1": np.int32, "tri_id2": np.int32}


def share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64; the library links the system one.  Whichever is loaded first serves both
    (same SONAME), and only PyTorch's copy works for PyTorch: import torch first whenever it is installed, so that tensors
    and the engine share one HIP runtime no matter in which order the application touches them."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib():
    """Loads the shared library (building it in-tree with hipcc if it is not there yet)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        from . import build as _build
        _build.build()
    share_hip_runtime_with_torch()
    L = ctypes.CDLL(LIB_PATH)
    u8p, f32p, i32p = ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p
    L.sv_params_init.argtypes = [ctypes.POINTER(SvParams), ctypes.c_int]
    L.sv_params_init.restype = None
    L.sv_create.argtypes = [ctypes.POINTER(SvParams), ctypes.POINTER(SvConfig), ctypes.POINTER(ctypes.c_void_p)]
    L.sv_create.restype = ctypes.c_int
    L.sv_destroy.argtypes = [ctypes.c_void_p]
    L.sv_destroy.restype = ctypes.c_int
    L.sv_last_error.argtypes = [ctypes.c_void_p]
    L.sv_last_error.restype = ctypes.c_char_p
    L.sv_wait.argtypes = [ctypes.c_void_p]
    L.sv_wait.restype = ctypes.c_int
    L.sv_wait_batches.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sv_wait_batches.restype = ctypes.c_int
    L.sv_host_alloc.argtypes = [ctypes.c_size_t]
    L.sv_host_alloc.restype = ctypes.c_void_p
    L.sv_host_free.argtypes = [ctypes.c_void_p]
    L.sv_host_free.restype = None
    L.sv_query.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sv_query.restype = ctypes.c_int
    for name in ("sv_process_batch_host_dmap", "sv_submit_batch_host_dmap"):
        f = getattr(L, name)
        f.argtypes = [ctypes.c_void_p, u8p, u8p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, i32p]
        f.restype = ctypes.c_int
    for name in ("sv_process_batch_device", "sv_process_batch_host", "sv_submit_batch_device", "sv_submit_batch_host"):
        f = getattr(L, name)
        f.argtypes = [ctypes.c_void_p, u8p, u8p, ctypes.c_int, ctypes.c_int, f32p, f32p, i32p]
        f.restype = ctypes.c_int
    L.sv_elas_process.argtypes = [ctypes.c_void_p, u8p, u8p, f32p, f32p, ctypes.POINTER(ctypes.c_int32)]
    L.sv_elas_process.restype = ctypes.c_int
    L.sv_debug_size.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.sv_debug_size.restype = ctypes.c_long
    L.sv_debug_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_long]
    L.sv_debug_get.restype = ctypes.c_long
    L.sv_kernel_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    L.sv_kernel_times.restype = ctypes.c_int
    L.sv_kernel_times_reset.argtypes = [ctypes.c_void_p]
    L.sv_kernel_times_reset.restype = None
    L.sv_kernel_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.sv_kernel_timing_enable.restype = None
    L.sv_kernel_timing_select.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.sv_kernel_timing_select.restype = ctypes.c_int
    L.sv_host_support_filter.argtypes = [ctypes.POINTER(SvParams), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    L.sv_host_support_filter.restype = ctypes.c_int
    L.sv_host_support_filter_threads.argtypes = [ctypes.POINTER(SvParams), ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.sv_host_support_filter_threads.restype = ctypes.c_int
    L.sv_host_delaunay.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    L.sv_host_delaunay.restype = ctypes.c_int
    _lib = L
    return L


class StereoError(RuntimeError):
    pass


class StereoEngine:
    """Batched Elas::process on one MI355X.

    engine = StereoEngine(1242, 375, SvParams.driver(127))
    d1, d2 = engine.process_device(left_u8_cuda, right_u8_cuda)     # torch tensors [B,H,W] -> float32 [B,H,W]
    """

    def __init__(self, width, height, params=None, device=0, n_workers=0, chunk=0, keep_debug=False, n_streams=0, n_slots=0, gpu_filter=None,
                 triangulation=None, resident=None, dg_sub_max=0, dg_max_points=0, affinity=None, inline=None, share_sliced=False, event_sync=None, latency_split=0, host_copies=None):
        """gpu_filter: None (automatic) / True / False - where the support-lattice filters run.  triangulation: None or "auto", "gpu", "host",
        "balanced" (by the pool's backlog, whatever its size) or an int 1..100 = that share of the chunks on the GPU.  resident / affinity /
        inline: None (automatic) or False to switch the resident GPU share / the NUMA binding / the calling-thread latency path off.
        dg_sub_max, dg_max_points: limits of the GPU triangulation (tests).  event_sync: None (automatic), "block", "spin" or "poll" - how the
        handle's threads wait for the GPU.  host_copies: None (automatic), "runtime" (hipMemcpyAsync) or "lanes" (engine-addressed SDMA copies) -
        who moves host-memory batches over PCIe.  See sv_config in include/stereo_vision_hip.h."""
        L = lib()
        self.params = params if params is not None else SvParams.driver(127)
        self.width, self.height, self.device = int(width), int(height), int(device)
        # disparity map size: half the image in half-resolution mode (Elas::parameters::subsampling, elas.h:83-85, 160-161)
        self.map_height, self.map_width = (self.height // 2, self.width // 2) if self.params.subsampling else (self.height, self.width)
        cfg = SvConfig(self.width, self.height, self.device, int(n_workers), int(chunk), int(bool(keep_debug)), int(n_streams), int(n_slots))
        cfg.gpu_lattice_filter = 0 if gpu_filter is None else (1 if gpu_filter else 2)
        if isinstance(triangulation, int) and not isinstance(triangulation, bool):
            cfg.gpu_triangulation, cfg.gpu_triangulation_pct = 3, int(triangulation)
        else:
            cfg.gpu_triangulation = _TRIANGULATION_MODES[triangulation]
        cfg.resident = 2 if resident is False else 0
        cfg.dg_sub_max, cfg.dg_max_points = int(dg_sub_max), int(dg_max_points)
        cfg.affinity = 2 if affinity is False else 0
        cfg.inline_latency_path = 2 if inline is False else 0
        cfg.share_sliced = int(bool(share_sliced))
        cfg.event_sync = {None: 0, "auto": 0, "block": 1, "spin": 2, "poll": 3}[event_sync]
        cfg.latency_split = int(latency_split)
        cfg.host_copies = {None: 0, "auto": 0, "runtime": 1, "lanes": 2}[host_copies]
        h = ctypes.c_void_p()
        rc = L.sv_create(ctypes.byref(self.params), ctypes.byref(cfg), ctypes.byref(h))
        if rc != 0:
            raise StereoError("sv_create failed (%d): %s" % (rc, L.sv_last_error(None).decode()))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().sv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def debug_set(self, key, value):
        """Test hooks on a live handle (sv_debug_set): "ccl_cap", "rt_cap", "host_force_staging", "ns_bound", "pool_sleep", "lat_trace", "dma_selftest_fail", "latency_pin", "lat_runtime_copies", "lat_filter_alone" (include/stereo_vision_hip.h)."""
        L = lib()
        L.sv_debug_set.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
        self._check(L.sv_debug_set(self._h, key.encode(), int(value)))

    def debug_inject(self, stage, left=None, right=None):
        """Test hook (sv_debug_inject): float32 [map_height, map_width] maps that replace dense_match's (stage "wta") or the L/R check's
        (stage "lr") for every later pair of this keep_debug handle; left = right = None clears them.  Stage "lattice" takes ONE int16
        [Hc, Wc] support lattice (left) that replaces the support matching's in front of the lattice filters.  The library refuses values
        the engine itself cannot produce at that stage (include/stereo_vision_hip.h)."""
        L = lib()
        L.sv_debug_inject.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
        L.sv_debug_inject.restype = ctypes.c_int
        if stage == "lattice" and left is not None:
            # the third stage (sv_debug_inject_lattice): ONE int16 [Hc, Wc] support lattice in place of the support matching's, in front
            # of the lattice filters; -1 or 0 .. disp_max, row 0 and column 0 zero
            if right is not None:
                raise ValueError("stage \"lattice\" takes one lattice")
            if not (isinstance(left, np.ndarray) and left.dtype == np.int16 and left.ndim == 2):
                raise ValueError("the lattice must be an int16 array [Hc,Wc]")
            lat = np.ascontiguousarray(left)
            L.sv_debug_inject_lattice.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
            L.sv_debug_inject_lattice.restype = ctypes.c_int
            return self._check(L.sv_debug_inject_lattice(self._h, lat.ctypes.data, lat.shape[1], lat.shape[0]))
        if left is None and right is None:
            return self._check(L.sv_debug_inject(self._h, stage.encode(), None, None))
        maps = []
        for m, name in ((left, "left"), (right, "right")):
            if not (isinstance(m, np.ndarray) and m.dtype == np.float32 and m.shape == (self.map_height, self.map_width)):
                raise ValueError("%s must be a float32 array [%d,%d]" % (name, self.map_height, self.map_width))
            maps.append(np.ascontiguousarray(m))
        self._check(L.sv_debug_inject(self._h, stage.encode(), maps[0].ctypes.data, maps[1].ctypes.data))

    def _check(self, rc):
        if rc != 0:
            raise StereoError("libstereo_vision_hip error %d: %s" % (rc, lib().sv_last_error(self._h).decode()))

    # ---- device path (inputs resident in HBM)
    def _check_device_batch(self, left, right, d1, d2, status):
        """The engine reads and writes raw pointers on its own streams: everything the kernels assume is checked here, and work
        pending on torch's current stream (an H2D copy of the inputs, a fill of the outputs) is waited for."""
        import torch
        dev = torch.device("cuda", self.device)
        for t, dt, name in ((left, torch.uint8, "left"), (right, torch.uint8, "right"), (d1, torch.float32, "d1"), (d2, torch.float32, "d2")):
            if t is None and name == "d2":
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev):
                raise ValueError("%s must be a CUDA tensor on %s (the handle's device)" % (name, dev))
            if t.dtype != dt or not t.is_contiguous() or t.dim() != 3:
                raise ValueError("%s must be a contiguous %s tensor [B,H,W]" % (name, dt))
        B = left.shape[0]
        if tuple(left.shape) != (B, self.height, self.width) or right.shape != left.shape:
            raise ValueError("images must be [B,%d,%d], got %s / %s" % (self.height, self.width, tuple(left.shape), tuple(right.shape)))
        for t, name in ((d1, "d1"), (d2, "d2")):
            if t is not None and tuple(t.shape) != (B, self.map_height, self.map_width):
                raise ValueError("%s must be [%d,%d,%d], got %s" % (name, B, self.map_height, self.map_width, tuple(t.shape)))
        if status is not None and not (isinstance(status, np.ndarray) and status.dtype == np.int32 and status.flags.c_contiguous and status.size >= B):
            raise ValueError("status must be a contiguous int32 numpy array with at least B entries")
        torch.cuda.current_stream(dev).synchronize()
        return B

    def process_device(self, left, right, d1=None, d2=None, want_d2=True, status=None):
        import torch
        if isinstance(left, torch.Tensor) and isinstance(right, torch.Tensor):
            left, right = left.contiguous(), right.contiguous()
        B = left.shape[0]
        if d1 is None:
            d1 = torch.zeros((B, self.map_height, self.map_width), dtype=torch.float32, device=left.device)
        if d2 is None and want_d2:
            d2 = torch.zeros((B, self.map_height, self.map_width), dtype=torch.float32, device=left.device)
        self._check_device_batch(left, right, d1, d2, status)
        st = status.ctypes.data_as(ctypes.c_void_p) if status is not None else None
        self._check(lib().sv_process_batch_device(self._h, left.data_ptr(), right.data_ptr(), B, self.width, d1.data_ptr(),
                                                  d2.data_ptr() if d2 is not None else None, st))
        return d1, d2

    def submit_device(self, left, right, d1, d2=None, status=None):
        """Streaming form: enqueue a device-resident batch and return at once (call wait() before touching d1/d2).
        Successive batches flow through the pipeline back to back."""
        B = self._check_device_batch(left, right, d1, d2, status)
        st = status.ctypes.data_as(ctypes.c_void_p) if status is not None else None
        self._check(lib().sv_submit_batch_device(self._h, left.data_ptr(), right.data_ptr(), B, self.width, d1.data_ptr(),
                                                 d2.data_ptr() if d2 is not None else None, st))

    def wait(self):
        self._check(lib().sv_wait(self._h))

    def wait_batches(self, n):
        """Returns when the n oldest batches submitted since the last wait() are complete; later ones keep running."""
        self._check(lib().sv_wait_batches(self._h, int(n)))

    # ---- host path (numpy in / out, PCIe inclusive): streamed through the pipeline, no allocation per call
    def _host_args(self, left, right, d1, d2, want_d2):
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        if left.ndim == 2:
            left, right = left[None], right[None]
        B, H, W = left.shape
        if (H, W) != (self.height, self.width) or right.shape != left.shape:
            raise ValueError("images must be [B,%d,%d]" % (self.height, self.width))
        shape = (B, self.map_height, self.map_width)
        if d1 is None:
            d1 = np.zeros(shape, np.float32)
        if d2 is None and want_d2:
            d2 = np.zeros(shape, np.float32)
        for m, name in ((d1, "d1"), (d2, "d2")):
            if m is not None and not (isinstance(m, np.ndarray) and m.dtype == np.float32 and m.flags.c_contiguous and m.shape == shape):
                raise ValueError("%s must be a contiguous float32 array %s" % (name, shape))
        return left, right, d1, d2, B

    def process_host(self, left, right, want_d2=True, d1=None, d2=None):
        """numpy [B,H,W] uint8 in, float32 maps out.  Page-locked arrays (pinned_array) skip the staging copies."""
        left, right, d1, d2, B = self._host_args(left, right, d1, d2, want_d2)
        status = np.zeros(B, np.int32)
        self._check(lib().sv_process_batch_host(self._h, left.ctypes.data, right.ctypes.data, B, self.width, d1.ctypes.data,
                                                d2.ctypes.data if d2 is not None else None, status.ctypes.data))
        return d1, d2, status

    def submit_host(self, left, right, d1, d2=None, status=None):
        """Streaming form of process_host: returns at once; the arrays must stay alive and untouched until wait()."""
        left_c, right_c, d1, d2, B = self._host_args(left, right, d1, d2, False)
        if left_c is not left and not np.shares_memory(left_c, left) or right_c is not right and not np.shares_memory(right_c, right):
            raise ValueError("submit_host needs contiguous uint8 arrays (a temporary copy would be freed before the engine reads it)")
        st = status.ctypes.data_as(ctypes.c_void_p) if status is not None else None
        self._check(lib().sv_submit_batch_host(self._h, left_c.ctypes.data, right_c.ctypes.data, B, self.width, d1.ctypes.data,
                                               d2.ctypes.data if d2 is not None else None, st))

    def _host_dmap_args(self, left, right, dmap):
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        if left.ndim == 2:
            left, right = left[None], right[None]
        B, H, W = left.shape
        if (H, W) != (self.height, self.width) or right.shape != left.shape:
            raise ValueError("images must be [B,%d,%d]" % (self.height, self.width))
        shape = (B, self.map_height, self.map_width)
        if dmap is None:
            dmap = np.zeros(shape, np.uint8)
        if not (isinstance(dmap, np.ndarray) and dmap.dtype == np.uint8 and dmap.flags.c_contiguous and dmap.shape == shape):
            raise ValueError("dmap must be a contiguous uint8 array %s" % (shape,))
        return left, right, dmap, B

    def process_host_dmap(self, left, right, dmap=None):
        """numpy [B,H,W] uint8 in, the driver's 8-bit disparity images out (saturate(round_half_even(4 * D1)), stereo_vision.cpp:316)."""
        left, right, dmap, B = self._host_dmap_args(left, right, dmap)
        status = np.zeros(B, np.int32)
        self._check(lib().sv_process_batch_host_dmap(self._h, left.ctypes.data, right.ctypes.data, B, self.width, dmap.ctypes.data, status.ctypes.data))
        return dmap, status

    def submit_host_dmap(self, left, right, dmap, status=None):
        """Streaming form of process_host_dmap: returns at once; the arrays must stay alive and untouched until wait()."""
        left_c, right_c, dmap, B = self._host_dmap_args(left, right, dmap)
        if left_c is not left and not np.shares_memory(left_c, left) or right_c is not right and not np.shares_memory(right_c, right):
            raise ValueError("submit_host_dmap needs contiguous uint8 arrays (a temporary copy would be freed before the engine reads it)")
        st = status.ctypes.data_as(ctypes.c_void_p) if status is not None else None
        self._check(lib().sv_submit_batch_host_dmap(self._h, left_c.ctypes.data, right_c.ctypes.data, B, self.width, dmap.ctypes.data, st))

    def elas_process(self, I1, I2):
        """Elas::process(I1, I2, D1, D2, dims) for one pair (elas.h:153-162)."""
        I1 = np.ascontiguousarray(I1, dtype=np.uint8)
        I2 = np.ascontiguousarray(I2, dtype=np.uint8)
        H, W = I1.shape
        D1 = np.zeros((self.map_height, self.map_width), np.float32)
        D2 = np.zeros((self.map_height, self.map_width), np.float32)
        dims = (ctypes.c_int32 * 3)(W, H, W)
        self._check(lib().sv_elas_process(self._h, I1.ctypes.data, I2.ctypes.data, D1.ctypes.data, D2.ctypes.data, dims))
        return D1, D2

    def debug(self, name):
        n = lib().sv_debug_size(self._h, name.encode())
        if n < 0:
            raise KeyError(name)
        dt = np.dtype(_STAGE_DTYPES.get(name, np.float32))
        out = np.empty(n // dt.itemsize, dtype=dt)
        got = lib().sv_debug_get(self._h, name.encode(), out.ctypes.data, n)
        assert got == n
        return out

    def query(self):
        """What the handle decided at creation: host threads, chunk, slots, where the lattice filters and the triangulations run."""
        L = lib()
        keys = ["host_threads", "chunk", "slots", "gpu_lattice_filter", "gpu_triangulation"]
        out = {k: int(L.sv_query(self._h, i)) for i, k in enumerate(keys)}
        out["numa_bound"] = int(L.sv_query(self._h, 7))
        out["resident"] = int(L.sv_query(self._h, 8))
        out["host_copies"] = int(L.sv_query(self._h, 9))  # 0 not decided yet (no host-memory batch so far), 1 hipMemcpyAsync, 2 DMA lanes
        out["latency_split"] = int(L.sv_query(self._h, 10))  # single pairs: triangulations on one thread each (0), in halves (1), in quarters (2)
        return out

    def gpu_triangulation_share(self):
        """Fraction of the pairs so far whose triangulations the GPU kernel built (host mode: the dispatcher's load balancing)."""
        return int(lib().sv_query(self._h, 5)) / 1000.0

    def gpu_triangulation_fallbacks(self):
        """Vertex sets of that share which the host triangulated after all (too large for the kernels)."""
        return int(lib().sv_query(self._h, 6))

    def timing(self, on=True, only=None):
        """HIP-event timing of the kernel launches; `only` = iterable of kernel names restricts it (cheaper)."""
        if lib().sv_kernel_timing_select(self._h, ",".join(only).encode() if only else None) != 0:
            raise ValueError("unknown kernel name in %r" % (only,))
        lib().sv_kernel_timing_enable(self._h, int(on))
        lib().sv_kernel_times_reset(self._h)

    def counters(self, enable=None):
        """Work counters of the matching kernels.  counters(True) enables and resets them, counters(False) disables;
        counters() returns {dense_candidates, dense_pixels, support_energies} since the last reset."""
        L = lib()
        L.sv_debug_counters.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        out = (ctypes.c_uint64 * 8)()
        self._check(L.sv_debug_counters(self._h, -1 if enable is None else int(bool(enable)), out))
        return {"dense_candidates": int(out[0]), "dense_pixels": int(out[1]), "support_energies": int(out[2]),
                "dense_band_full": int(out[3]), "dense_band_partial": int(out[4]), "dense_band_per_lane": int(out[5]),
                "dense_grid_wave_trips": int(out[6]), "dense_grid_lane_trips": int(out[7])}

    def kernel_times(self):
        """{kernel: (total_ms, calls)} accumulated since timing(True)."""
        cap = 64
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_double * cap)()
        calls = (ctypes.c_int64 * cap)()
        n = lib().sv_kernel_times(self._h, names, ms, calls, cap)
        return {names[i].decode(): (ms[i], calls[i]) for i in range(n)}


class _PinnedBlock:
    def __init__(self, nbytes):
        self.ptr = lib().sv_host_alloc(max(int(nbytes), 1))
        if not self.ptr:
            raise StereoError("sv_host_alloc(%d) failed" % nbytes)

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                lib().sv_host_free(self.ptr)
            except TypeError:  # interpreter shutdown: the module globals are already gone (the process's memory goes with it)
                pass
            self.ptr = None


def pinned_array(shape, dtype):
    """numpy array in page-locked host memory (sv_host_alloc): the engine's host path moves it by DMA without a staging copy.
    The memory lives as long as the array (or any view of it)."""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    block = _PinnedBlock(n)
    buf = (ctypes.c_uint8 * max(n, 1)).from_address(block.ptr)
    buf._sv_block = block  # keeps the allocation alive: the array's base chain holds the ctypes buffer
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def reproject(disp, Q, XR=None, XT=None, want_dmap=True):
    """Batched disparity -> (u8 x4 map, 3-D points) on the device (stereo_vision.cpp:316, :233-256; optional robot-frame transform of
    the CUDA variant).  disp: CUDA float32 tensor [B,H,W]; Q: 4x4; returns (dmap uint8 [B,H,W] or None, points float64 [B,H,W,3])."""
    import torch
    assert disp.is_cuda and disp.dtype == torch.float32 and disp.dim() == 3
    disp = disp.contiguous()
    B, H, W = disp.shape
    q, xr, xt = _reproject_pointers(Q, XR, XT)
    dmap = torch.empty((B, H, W), dtype=torch.uint8, device=disp.device) if want_dmap else None
    pts = torch.empty((B, H, W, 3), dtype=torch.float64, device=disp.device)
    torch.cuda.current_stream(disp.device).synchronize()
    L = lib()
    L.sv_reproject_batch_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p]
    with torch.cuda.device(disp.device):
        rc = L.sv_reproject_batch_device(disp.data_ptr(), B, W, H, q, xr, xt, dmap.data_ptr() if dmap is not None else None, pts.data_ptr())
    if rc != 0:
        raise StereoError("sv_reproject_batch_device failed (%d)" % rc)
    return dmap, pts


def disparity_to_u8(disp, out=None):
    """The driver's 8-bit disparity image (saturate(round_half_even(4 * d)), stereo_vision.cpp:316) of a CUDA float32 tensor, on torch's
    current stream (not waited for)."""
    import torch
    assert disp.is_cuda and disp.dtype == torch.float32 and disp.is_contiguous()
    if out is None:
        out = torch.empty(disp.shape, dtype=torch.uint8, device=disp.device)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == disp.numel()
    L = lib()
    L.sv_disparity_to_u8_device.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p]
    with torch.cuda.device(disp.device):
        rc = L.sv_disparity_to_u8_device(disp.data_ptr(), disp.numel(), out.data_ptr(), torch.cuda.current_stream(disp.device).cuda_stream)
    if rc != 0:
        raise StereoError("sv_disparity_to_u8_device failed (%d)" % rc)
    return out


class SvTopViewSpec(ctypes.Structure):
    """sv_top_view_spec of include/stereo_vision_hip.h."""
    _fields_ = [("x_range", ctypes.c_double * 2), ("y_range", ctypes.c_double * 2), ("z_range", ctypes.c_double * 2), ("scale", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("disparity", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


class SvBoxSpec(ctypes.Structure):
    """sv_box_spec of include/stereo_vision_hip.h."""
    _fields_ = [("select", ctypes.c_int32), ("disparity", ctypes.c_int32), ("band", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


class SvCloudSpec(ctypes.Structure):
    """sv_cloud_spec of include/stereo_vision_hip.h."""
    _fields_ = [("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3), ("disparity", ctypes.c_int32), ("step", ctypes.c_int32),
                ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


class SvVoxelSpec(ctypes.Structure):
    """sv_voxel_spec of include/stereo_vision_hip.h."""
    _fields_ = [("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3), ("size", ctypes.c_double), ("disparity", ctypes.c_int32),
                ("step", ctypes.c_int32), ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


class SvGroundSpec(ctypes.Structure):
    """sv_ground_spec of include/stereo_vision_hip.h."""
    _fields_ = [("n_bins", ctypes.c_int32), ("vh_lo", ctypes.c_int32), ("vh_hi", ctypes.c_int32), ("vh_step", ctypes.c_int32),
                ("qb_step", ctypes.c_int32), ("tol", ctypes.c_int32), ("g_tol", ctypes.c_int32), ("min_run", ctypes.c_int32),
                ("min_support", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7)]


class SvStixelSpec(ctypes.Structure):
    """sv_stixel_spec of include/stereo_vision_hip.h."""
    _fields_ = [("n_bins", ctypes.c_int32), ("q_min", ctypes.c_int32), ("sim", ctypes.c_int32), ("max_gap", ctypes.c_int32),
                ("min_rows", ctypes.c_int32), ("max_layers", ctypes.c_int32), ("col_step", ctypes.c_int32), ("sim_cols", ctypes.c_int32),
                ("min_cols", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7)]


class SvOccupancySpec(ctypes.Structure):
    """sv_occupancy_spec of include/stereo_vision_hip.h."""
    _fields_ = [("x_range", ctypes.c_double * 2), ("y_range", ctypes.c_double * 2), ("z_range", ctypes.c_double * 2), ("scale", ctypes.c_int32),
                ("z_scale", ctypes.c_int32), ("min_obstacle", ctypes.c_int32), ("min_ground", ctypes.c_int32), ("min_rays", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 5)]


class SvOccupancyMapSpec(ctypes.Structure):
    """sv_occupancy_map_spec of include/stereo_vision_hip.h."""
    _fields_ = [("top", ctypes.c_int32), ("left", ctypes.c_int32), ("rows", ctypes.c_int32), ("cols", ctypes.c_int32), ("scale", ctypes.c_int32),
                ("l_occ", ctypes.c_int32), ("l_free", ctypes.c_int32), ("l_min", ctypes.c_int32), ("l_max", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7)]


class SvVoxelMapSpec(ctypes.Structure):
    """sv_voxel_map_spec of include/stereo_vision_hip.h."""
    _fields_ = [("lo", ctypes.c_double * 3), ("hi", ctypes.c_double * 3), ("size", ctypes.c_double), ("capacity", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 7)]


class SvVoxelRenderSpec(ctypes.Structure):
    """sv_voxel_render_spec of include/stereo_vision_hip.h."""
    _fields_ = [("f", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double), ("q32", ctypes.c_double), ("q33", ctypes.c_double),
                ("half_px", ctypes.c_double), ("near", ctypes.c_double), ("far", ctypes.c_double), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("r_max", ctypes.c_int32), ("reserved", ctypes.c_int32 * 5)]


class SvVoxelFlattenSpec(ctypes.Structure):
    """sv_voxel_flatten_spec of include/stereo_vision_hip.h."""
    _fields_ = [("mode", ctypes.c_int32), ("z_ref_q", ctypes.c_int32), ("step_q", ctypes.c_int32), ("height_q", ctypes.c_int32), ("radius", ctypes.c_int32),
                ("min_obstacle", ctypes.c_int32), ("min_ground", ctypes.c_int32), ("reserved", ctypes.c_int32 * 9)]


class SvVoxelClusterSpec(ctypes.Structure):
    """sv_voxel_cluster_spec of include/stereo_vision_hip.h."""
    _fields_ = [("connectivity", ctypes.c_int32), ("mode", ctypes.c_int32), ("z_ref_q", ctypes.c_int32), ("h_lo_q", ctypes.c_int32), ("h_hi_q", ctypes.c_int32),
                ("min_voxels", ctypes.c_int32), ("capacity", ctypes.c_int32), ("drop", ctypes.c_int32), ("reserved", ctypes.c_int32 * 8)]


class SvFlowSpec(ctypes.Structure):
    """sv_flow_spec of include/stereo_vision_hip.h."""
    _fields_ = [("f", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double), ("b16", ctypes.c_double), ("fb", ctypes.c_double), ("fb16", ctypes.c_double),
                ("step", ctypes.c_int32), ("r", ctypes.c_int32), ("wx", ctypes.c_int32), ("wy", ctypes.c_int32), ("ratio", ctypes.c_int32), ("max_cost", ctypes.c_int32),
                ("capacity", ctypes.c_int32), ("reserved", ctypes.c_int32 * 9)]


class SvWarpSpec(ctypes.Structure):
    """sv_warp_spec of include/stereo_vision_hip.h."""
    _fields_ = [("f", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double), ("b16", ctypes.c_double), ("fb", ctypes.c_double), ("fb16", ctypes.c_double),
                ("e_max", ctypes.c_int32), ("tol_q", ctypes.c_int32), ("rel_q", ctypes.c_int32), ("mode", ctypes.c_int32), ("reserved", ctypes.c_int32 * 12)]


class SvTrackSpec(ctypes.Structure):
    """sv_track_spec of include/stereo_vision_hip.h."""
    _fields_ = [("f", ctypes.c_double), ("cx", ctypes.c_double), ("cy", ctypes.c_double), ("b16", ctypes.c_double), ("fb", ctypes.c_double), ("fb16", ctypes.c_double),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("max_boxes", ctypes.c_int32), ("band_q", ctypes.c_int32), ("min_votes", ctypes.c_int32),
                ("share", ctypes.c_int32), ("gate_m", ctypes.c_int32), ("reserved", ctypes.c_int32 * 9)]


class SvPlaceSpec(ctypes.Structure):
    """sv_place_spec of include/stereo_vision_hip.h."""
    _fields_ = [("r_max", ctypes.c_double), ("z_lo", ctypes.c_double), ("z_hi", ctypes.c_double), ("r_min", ctypes.c_double),
                ("rings", ctypes.c_int32), ("sectors", ctypes.c_int32), ("reserved", ctypes.c_int32 * 10)]


class SvPoseGraphSpec(ctypes.Structure):
    """sv_pose_graph_spec of include/stereo_vision_hip.h (AE)."""
    _fields_ = [("lam", ctypes.c_double), ("tol", ctypes.c_double), ("reserved", ctypes.c_int32 * 12)]


def _signatures():
    """The table below: per stage group of the C API, (D) to (S), its functions and per function (restype, argtypes), parameter by
    parameter as include/stereo_vision_hip.h declares them - tests/test_stage_signatures.py holds the two against each other."""
    P = ctypes.POINTER
    vp, ci, sz, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_int64
    tv, bx, cl, vx, gr, sx = P(SvTopViewSpec), P(SvBoxSpec), P(SvCloudSpec), P(SvVoxelSpec), P(SvGroundSpec), P(SvStixelSpec)
    oc, om, vm = P(SvOccupancySpec), P(SvOccupancyMapSpec), P(SvVoxelMapSpec)
    return {
        "top_view": {  # (D)
            "sv_top_view_dims": (ci, [tv, P(ci), P(ci)]),
            "sv_top_view_workspace_bytes": (sz, [tv, ci]),
            "sv_top_view_points_device": (ci, [vp, ci, i64, tv, vp, vp, sz, vp]),
            "sv_top_view_disparity_device": (ci, [vp, ci, ci, ci, vp, vp, vp, tv, vp, vp, sz, vp]),
            "sv_debug_top_view": (ci, [ci, vp]),
        },
        "box": {  # (E)
            "sv_box_positions_disparity_device": (ci, [vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, bx, vp, vp, vp]),
            "sv_box_positions_points_device": (ci, [vp, ci, ci, ci, vp, vp, ci, bx, vp, vp, vp]),
        },
        "cloud": {  # (F)
            "sv_cloud_tile": (ci, []),
            "sv_cloud_workspace_bytes": (sz, [cl, ci, ci, ci]),
            "sv_cloud_disparity_device": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, cl, ci, vp, vp, vp, vp, vp, sz, vp]),
        },
        "ground": {  # (G)
            "sv_ground_workspace_bytes": (sz, [gr, ci, ci, ci]),
            "sv_ground_disparity_device": (ci, [vp, ci, ci, ci, gr, vp, vp, vp, vp, vp, vp, sz, vp]),
        },
        "stixel": {  # (H)
            "sv_stixel_workspace_bytes": (sz, [sx, ci, ci, ci]),
            "sv_stixel_disparity_device": (ci, [vp, vp, ci, ci, ci, sx, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
        },
        "voxel": {  # (I)
            "sv_voxel_table_slots": (i64, [ci]),
            "sv_voxel_workspace_bytes": (sz, [vx, ci, ci, ci, ci]),
            "sv_voxel_disparity_device": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, vx, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
            "sv_debug_voxel": (ci, [ci, vp]),
        },
        "occupancy": {  # (J)
            "sv_occupancy_dims": (ci, [oc, P(ci), P(ci)]),
            "sv_occupancy_disparity_device": (ci, [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, oc, vp, vp, vp, vp]),
            "sv_debug_occupancy": (ci, [ci, vp]),
        },
        "occupancy_map": {  # (K)
            "sv_occupancy_fuse_device": (ci, [vp, vp, ci, ci, oc, om, ci, ci, vp, vp, vp, vp, vp]),
            "sv_debug_occupancy_fuse": (ci, [ci, vp]),
        },
        "map_match": {  # (L)
            "sv_map_match_workspace": (ci, [oc, ci, ci, P(sz)]),
            "sv_map_match_device": (ci, [vp, vp, ci, ci, oc, om, vp, ci, ci, vp, vp, vp, vp, vp, sz, vp]),
            "sv_debug_map_match": (ci, [ci, vp]),
        },
        "clearance": {  # (M)
            "sv_clearance_workspace": (ci, [ci, ci, P(sz)]),
            "sv_clearance_device": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, sz, vp]),
            "sv_clearance_paths_device": (ci, [vp, om, vp, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp]),
            "sv_debug_clearance": (ci, [ci, vp]),
        },
        "cost": {  # (N)
            "sv_cost_cells_device": (ci, [vp, ci, ci, ci, ci, ci, ci, vp, vp]),
            "sv_cost_to_goal_workspace": (ci, [ci, ci, P(sz)]),
            "sv_cost_to_goal_device": (ci, [vp, ci, ci, vp, ci, ci, ci, vp, vp, sz, vp, vp]),
            "sv_cost_routes_device": (ci, [vp, vp, ci, ci, vp, ci, ci, vp, vp, vp, vp]),
            "sv_debug_cost_to_goal": (ci, [ci, vp]),
        },
        "frontier": {  # (O)
            "sv_frontier_cells_device": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, vp]),
            "sv_frontier_clusters_workspace": (ci, [ci, ci, ci, P(sz)]),
            "sv_frontier_clusters_device": (ci, [vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, sz, vp]),
            "sv_debug_frontier": (ci, [ci, vp]),
        },
        "view": {  # (P)
            "sv_view_workspace": (ci, [ci, ci, P(sz)]),
            "sv_view_device": (ci, [vp, vp, om, vp, ci, ci, vp, ci, ci, ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, vp]),
            "sv_debug_view": (ci, [ci, ci]),
        },
        "voxel_map": {  # (Q)
            "sv_voxel_map_slots": (i64, [ci]),
            "sv_voxel_map_bytes": (sz, [ci]),
            "sv_voxel_map_slot_of": (i64, [i64, i64]),
            "sv_voxel_map_clear_device": (ci, [vp, sz, vm, vp]),
            "sv_voxel_map_insert_device": (ci, [vp, sz, vm, vp, ci, vp, vp, vp, vp, ci, ci, ci, vp]),
            "sv_voxel_map_rows_device": (ci, [vp, sz, vm, i64, i64, ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "sv_debug_voxel_map": (ci, [ci, vp]),
        },
        "voxel_match": {  # (R)
            "sv_voxel_match_workspace": (ci, [ci, ci, ci, P(sz)]),
            "sv_voxel_match_device": (ci, [vp, sz, vm, vp, ci, vp, vp, vp, ci, ci, ci, i64, i64, ci, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
            "sv_debug_voxel_match": (ci, [ci]),
        },
        "voxel_carry": {  # (S)
            "sv_voxel_map_carry_device": (ci, [vp, sz, vm, vp, sz, vm, ci, ci, ci, i64, i64, ci, vp, vp]),
        },
        "voxel_carve": {  # (T)
            "sv_voxel_carve_device": (ci, [vp, sz, vm, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, i64, ci, ci, vp, vp, vp]),
        },
        "voxel_render": {  # (U)
            "sv_voxel_render_device": (ci, [vp, sz, vm, P(SvVoxelRenderSpec), vp, ci, i64, i64, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "sv_debug_voxel_render": (ci, [ci, ci]),
        },
        "voxel_flatten": {  # (V)
            "sv_voxel_flatten_device": (ci, [vp, sz, vm, om, P(SvVoxelFlattenSpec), i64, i64, ci, vp, vp, vp, vp, vp, vp, vp]),
            "sv_debug_voxel_flatten": (ci, [ci, ci]),
        },
        "voxel_clusters": {  # (W)
            "sv_voxel_clusters_workspace_bytes": (sz, [i64, ci]),
            "sv_voxel_clusters_device": (ci, [vp, sz, vm, P(SvVoxelClusterSpec), om, vp, i64, i64, ci, vp, vp, vp, vp, sz, vp]),
            "sv_debug_voxel_clusters": (ci, [ci, ci]),
        },
        "voxel_align": {  # (X)
            "sv_voxel_align_workspace": (ci, [ci, ci, P(sz)]),
            "sv_voxel_align_device": (ci, [vp, sz, vm, vp, ci, vp, vp, vp, vp, ci, ci, ci, i64, i64, ci, vp, vp, vp, vp, sz, vp]),
            "sv_debug_voxel_align": (ci, [ci, ci]),
        },
        "voxel_normals": {  # (Y)
            "sv_voxel_normals_device": (ci, [vp, sz, vm, vp, ci, ci, ci, ci, i64, i64, ci, vp, i64, vp, vp, vp]),
            "sv_voxel_plane_align_workspace": (ci, [ci, ci, P(sz)]),
            "sv_voxel_plane_align_device": (ci, [vp, sz, vm, vp, ci, vp, vp, vp, vp, ci, ci, ci, i64, i64, ci, vp, i64, vp, ci, vp, vp, vp, vp, vp, sz, vp]),
            "sv_debug_voxel_normals": (ci, [ci, ci]),
        },
        "flow": {  # (Z)
            "sv_flow_match_workspace": (ci, [ci, ci, ci, P(SvFlowSpec), P(sz)]),
            "sv_flow_match_device": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, P(SvFlowSpec), vp, vp, vp, vp, sz, vp]),
            "sv_flow_pose_sums_workspace": (ci, [ci, ci, P(sz)]),
            "sv_flow_pose_sums_device": (ci, [vp, vp, vp, ci, ci, P(SvFlowSpec), ci, ci, vp, vp, sz, vp]),
        },
        "warp": {  # (AA)
            "sv_disparity_warp_workspace": (ci, [ci, ci, ci, P(sz)]),
            "sv_disparity_warp_device": (ci, [vp, vp, vp, ci, ci, ci, P(SvWarpSpec), vp, vp, vp, vp, vp, vp, sz, vp]),
        },
        "track": {  # (AB)
            "sv_object_links_workspace": (ci, [ci, ci, P(sz)]),
            "sv_object_links_device": (ci, [vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, P(SvTrackSpec), vp, vp, vp, vp, sz, vp]),
            "sv_debug_object_links": (ci, [ci]),
        },
        "place": {  # (AC)
            "sv_place_descriptor_workspace": (ci, [ci, ci, ci, P(sz)]),
            "sv_place_descriptor_device": (ci, [vp, ci, vp, vp, vp, ci, ci, vp, P(SvPlaceSpec), vp, vp, vp, vp, sz, vp]),
            "sv_place_match_workspace": (ci, [ci, ci, P(sz)]),
            "sv_place_match_device": (ci, [vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]),
            "sv_debug_place": (ci, [ci]),
        },
        "voxel_repose": {  # (AD)
            "sv_voxel_repose_device": (ci, [vp, sz, vm, vp, sz, vm, vp, ci, ci, i64, i64, ci, vp, vp]),
        },
        "pose_graph": {  # (AE)
            "sv_pose_graph_linearize_device": (ci, [vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, P(SvPoseGraphSpec), vp, vp, vp, vp, vp, vp]),
            "sv_pose_graph_workspace": (ci, [ci, ci, P(sz)]),
            "sv_pose_graph_pcg_device": (ci, [vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, vp, P(SvPoseGraphSpec), ci, ci, vp, vp, sz, vp]),
        },
    }


STAGE_SIGNATURES = _signatures()  # plain data: made without loading the library
_GROUP_NEEDS = {"voxel": ("cloud",), "occupancy_map": ("occupancy",), "map_match": ("occupancy_map",), "clearance": ("occupancy_map",), "cost": ("clearance",), "frontier": ("cost",)}
_GROUP_NEEDS["view"] = ("occupancy_map",)
_GROUP_NEEDS["voxel_match"] = ("voxel_map",)
_GROUP_NEEDS["voxel_carry"] = ("voxel_map",)
_GROUP_NEEDS["voxel_carve"] = ("voxel_map",)
_GROUP_NEEDS["voxel_render"] = ("voxel_map",)
_GROUP_NEEDS["voxel_flatten"] = ("voxel_map", "occupancy_map")
_GROUP_NEEDS["voxel_clusters"] = ("voxel_map", "occupancy_map")
_GROUP_NEEDS["voxel_align"] = ("voxel_map",)
_GROUP_NEEDS["voxel_normals"] = ("voxel_map",)
_GROUP_NEEDS["voxel_repose"] = ("voxel_map",)
_bound_groups = set()


def _bind(group):
    """The library with the signatures of `group`, and of the groups its callers use with it, declared.  Group by group and only when one
    is first asked for: a library under SV_LIB_PATH that lacks a later group still loads and serves the earlier ones."""
    L = lib()
    if group not in _bound_groups:
        for g in _GROUP_NEEDS.get(group, ()):
            _bind(g)
        for name, (restype, argtypes) in STAGE_SIGNATURES[group].items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        _bound_groups.add(group)
    return L


def _check(rc, name, text=True):
    """Raises for a non-zero return code of the C entry `name` - ValueError for SV_ERR_ARG (-1), StereoError for anything else - with the
    text the entry left for sv_last_error(NULL).  text=False for group (D), whose entries leave none: what another call left there is
    not theirs."""
    if rc != 0:
        msg = "%s failed (%d)" % (name, rc)
        if text:
            msg += ": " + (lib().sv_last_error(None) or b"").decode()
        raise ValueError(msg) if rc == -1 else StereoError(msg)


def _ptr(t):
    """The device pointer of an optional output: NULL for None and for a tensor without elements."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _reproject_pointers(Q, XR=None, XT=None):
    """-> Q16, XR9, XT3 as a C entry takes them: pointers to contiguous float64 copies (None for an XR / XT not given), each of which
    holds its array for as long as it lives - keep them until the call has returned."""
    return [None if m is None else np.ascontiguousarray(m, dtype=np.float64).reshape(n).ctypes.data_as(ctypes.c_void_p)
            for m, n in ((Q, 16), (XR, 9), (XT, 3))]


def _disparity_batch(t, name, max_rows=None, one_frame=True):
    """The disparity maps of a stage, checked for what every kernel assumes -> (the contiguous CUDA float32 [B,H,W] tensor, whether it
    was one frame [H,W] that got its B here).  max_rows: the stage's own limit on H, if it has one."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() in ((2, 3) if one_frame else (3,))):
        raise ValueError("%s must be a CUDA float32 tensor [B,H,W]" % name)
    one = t.dim() == 2
    t = (t.unsqueeze(0) if one else t).contiguous()
    B, H, W = t.shape
    if B > 65535 or H < 1 or W < 1 or H * W >= 2 ** 31 or (max_rows is not None and H > max_rows):
        raise ValueError("%s: at most 65535 pairs of 1 <= width * height < 2^31 pixels%s, got %s"
                         % (name, "" if max_rows is None else " and at most %d rows" % max_rows, tuple(t.shape)))
    return t, one


def _colors_batch(colors, d1):
    """The colour images of a cloud stage, checked against its maps d1 [B,H,W] -> None, or the contiguous CUDA uint8 [B,H,W,4] tensor the
    C entry wants: 4-byte aligned, so a view that starts at an odd storage offset is copied."""
    import torch
    if colors is None:
        return None
    if not (isinstance(colors, torch.Tensor) and colors.is_cuda and colors.dtype == torch.uint8 and colors.device == d1.device):
        raise ValueError("colors must be a CUDA uint8 tensor [B,H,W,4] on d1's device")
    colors = (colors.unsqueeze(0) if colors.dim() == 3 else colors).contiguous()
    if tuple(colors.shape) != tuple(d1.shape) + (4,):
        raise ValueError("colors must be [B,H,W,4] matching d1 %s, got %s" % (tuple(d1.shape), tuple(colors.shape)))
    if colors.data_ptr() % 4:  # the C entry moves a pixel as one dword
        colors = colors.clone()
    return colors


class _Result:
    """What the result classes below share: every slot is set from the keyword of its name, None where none is given."""
    __slots__ = ()

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


_TOP_VIEW_MODES = {"reference": 0, "count": 1}
_TOP_VIEW_DISPARITY = {"dmap": 0, "d1": 1}


def top_view_lib():
    """The library with the sv_top_view_* signatures declared."""
    return _bind("top_view")


def top_view_spec(x_range, y_range, z_range, scale, mode="reference", disparity="dmap"):
    """-> (SvTopViewSpec, rows, cols); ValueError for a bad argument (the checks of sv_top_view_dims, made in Python first)."""
    from .stereo_vision.sv import top_view_grid
    rows, cols = top_view_grid(x_range, y_range, z_range, scale, mode)
    if disparity not in _TOP_VIEW_DISPARITY:
        raise ValueError("disparity must be one of %s, got %r" % (sorted(_TOP_VIEW_DISPARITY), disparity))
    spec = SvTopViewSpec()
    spec.x_range[:] = [float(v) for v in x_range]
    spec.y_range[:] = [float(v) for v in y_range]
    spec.z_range[:] = [float(v) for v in z_range]
    spec.scale, spec.mode, spec.disparity = int(scale), _TOP_VIEW_MODES[mode], _TOP_VIEW_DISPARITY[disparity]
    return spec, rows, cols


def _top_view_buffers(spec, B, rows, cols, device):
    """The grid (u8 or int32 [B,rows,cols]) and the reference mode's key workspace, from torch's allocator."""
    import torch
    out = torch.empty((B, rows, cols), dtype=torch.uint8 if spec.mode == 0 else torch.int32, device=device)
    nbytes = top_view_lib().sv_top_view_workspace_bytes(ctypes.byref(spec), B)
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device) if nbytes else None
    return out, ws, nbytes


def top_view(points, x_range, y_range, z_range, scale, mode="reference"):
    """Bird's-eye views of a batch of clouds on the device: points is a CUDA float64 tensor [B,...,3] (e.g. rig.point_clouds' [B,H,W,3]),
    each frame's points in flat order.  Returns a CUDA tensor [B,rows,cols], uint8 (mode "reference") or int32 (mode "count"), equal
    to stereo_vision.sv.points_2_top_view of each frame.  Enqueued on torch's current stream (not waited for)."""
    import torch
    spec, rows, cols = top_view_spec(x_range, y_range, z_range, scale, mode)
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float64 and points.dim() >= 3 and points.shape[-1] == 3):
        raise ValueError("points must be a CUDA float64 tensor [B,...,3]")
    B = points.shape[0]
    pts = points.contiguous()
    n = pts.numel() // (3 * B) if B else 0
    out, ws, nbytes = _top_view_buffers(spec, B, rows, cols, pts.device)
    with torch.cuda.device(pts.device):
        rc = top_view_lib().sv_top_view_points_device(pts.data_ptr(), B, n, ctypes.byref(spec), out.data_ptr(), _ptr(ws), nbytes,
                                                      torch.cuda.current_stream(pts.device).cuda_stream)
    _check(rc, "sv_top_view_points_device", text=False)
    return out


def top_view_from_disparity(disp, Q, x_range, y_range, z_range, scale, XR=None, XT=None, disparity="dmap", mode="reference"):
    """Bird's-eye views straight from disparity maps (CUDA float32 [B,H,W]): each pixel's point is reproject()'s, computed in registers,
    and no cloud is written.  disparity "dmap" reprojects the driver's saturate(round(4 d)) - the grid of top_view(reproject(disp, Q, XR,
    XT)[1]), whose points are at a quarter of metric depth (the driver's convention) -; "d1" reprojects d itself (metres) and skips
    pixels with d <= 0.  Returns what top_view returns; enqueued on torch's current stream."""
    import torch
    spec, rows, cols = top_view_spec(x_range, y_range, z_range, scale, mode, disparity)
    disp, _ = _disparity_batch(disp, "disp", 65535, one_frame=False)
    B, H, W = disp.shape
    q, xr, xt = _reproject_pointers(Q, XR, XT)
    out, ws, nbytes = _top_view_buffers(spec, B, rows, cols, disp.device)
    with torch.cuda.device(disp.device):
        rc = top_view_lib().sv_top_view_disparity_device(disp.data_ptr(), B, W, H, q, xr, xt, ctypes.byref(spec), out.data_ptr(), _ptr(ws), nbytes,
                                                         torch.cuda.current_stream(disp.device).cuda_stream)
    _check(rc, "sv_top_view_disparity_device", text=False)
    return out


def box_lib():
    """The library with the sv_box_positions_* signatures declared."""
    return _bind("box")


def box_spec(select="near", disparity="d1", band=4):
    """-> SvBoxSpec; ValueError for a bad argument (the checks of the C entry, made in Python first)."""
    from .stereo_vision.sv import BOX_DISPARITY, BOX_SELECT
    if select not in BOX_SELECT:
        raise ValueError("select must be one of %s, got %r" % (sorted(BOX_SELECT), select))
    if disparity not in BOX_DISPARITY:
        raise ValueError("disparity must be one of %s, got %r" % (sorted(BOX_DISPARITY), disparity))
    if isinstance(band, bool) or int(band) != band or not 0 <= band < 2 ** 31:
        raise ValueError("band must be an integer >= 0, got %r" % (band,))
    return SvBoxSpec(BOX_SELECT[select], BOX_DISPARITY[disparity], int(band))


def _box_buffers(boxes, n_boxes, B, device):
    """-> (boxes int32 [B,M,4] on the device, n_boxes int32 [B] there or None, pos pre-filled with NaN, stat with -1)."""
    import torch

    def dev(x, what):
        if isinstance(x, torch.Tensor):
            if x.is_floating_point():
                raise ValueError("%s must be integers" % what)
            return x.to(device=device, dtype=torch.int32).contiguous()
        a = np.asarray(x)
        if a.dtype.kind not in "iu":
            raise ValueError("%s must be integers" % what)
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)

    bx = dev(boxes, "boxes")
    if bx.dim() == 2 and B == 1:
        bx = bx.unsqueeze(0)
    if bx.dim() != 3 or bx.shape[0] != B or bx.shape[2] != 4:
        raise ValueError("boxes must be int32 [B,M,4] with B = %d (one frame: [M,4]), got shape %s" % (B, tuple(bx.shape)))
    M = bx.shape[1]
    if B > 65535 or M > 65535:
        raise ValueError("at most 65535 pairs and 65535 boxes per pair")
    nb = None
    if n_boxes is not None:
        nb = dev(n_boxes, "n_boxes").reshape(-1)
        if nb.numel() != B:
            raise ValueError("n_boxes must have one entry per pair (%d), got %d" % (B, nb.numel()))
    pos = torch.full((B, M, 3), float("nan"), dtype=torch.float64, device=device)
    stat = torch.full((B, M, 4), -1, dtype=torch.int32, device=device)
    return bx, nb, pos, stat


def box_positions(points, boxes, n_boxes=None):
    """Mean point of a batch of clouds inside detector boxes, on the device: points is a CUDA float64 tensor [B,H,W,3] (e.g.
    rig.point_clouds' or reproject's; one frame [H,W,3] accepted), boxes int32 [B,M,4] = (x, y, w, h) (CUDA tensor or numpy; [M,4] for
    one frame), n_boxes [B] = boxes in use per pair or None = all M.  Returns (pos float64 [B,M,3], stat int32 [B,M,4] = (n_pixels, -1,
    -1, n_pixels)) CUDA tensors equal to stereo_vision.sv.box_positions(points, boxes, n_boxes) - every pixel of the box, the
    reference's mean (inf / NaN propagate) in the library's summation order; rows at and beyond n_boxes[b] are NaN / -1.  Enqueued on
    torch's current stream (not waited for)."""
    import torch
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float64 and points.dim() in (3, 4) and points.shape[-1] == 3):
        raise ValueError("points must be a CUDA float64 tensor [B,H,W,3]")
    pts = (points.unsqueeze(0) if points.dim() == 3 else points).contiguous()
    B, H, W = pts.shape[:3]
    spec = box_spec("all", "dmap", 0)
    bx, nb, pos, stat = _box_buffers(boxes, n_boxes, B, pts.device)
    with torch.cuda.device(pts.device):
        rc = box_lib().sv_box_positions_points_device(pts.data_ptr(), B, W, H, bx.data_ptr(), _ptr(nb), bx.shape[1], ctypes.byref(spec),
                                                      pos.data_ptr(), stat.data_ptr(), torch.cuda.current_stream(pts.device).cuda_stream)
    _check(rc, "sv_box_positions_points_device")
    return pos, stat


def box_positions_from_disparity(disp, Q, boxes, n_boxes=None, XR=None, XT=None, select="near", disparity="d1", band=4):
    """Object positions straight from disparity maps (CUDA float32 [B,H,W]; one frame [H,W] accepted): each pixel's point is reproject()'s,
    computed in registers, and no cloud is written.  disparity "dmap": the driver's saturate(round(4 d)) reprojected (a quarter of metric
    depth), valid where it is > 0; "d1": d itself (metres), valid where d > 0.  select "all": every pixel of the box (with "dmap":
    box_positions(reproject(disp, Q, XR, XT)[1], boxes), bit for bit); "valid": the valid pixels; "near": the valid pixels within `band`
    quarter pixels of the box's lower-median quantised disparity.  Returns (pos float64 [B,M,3], stat int32 [B,M,4] = (n_pixels,
    n_valid, q_med, n_selected)) equal to stereo_vision.sv.box_positions(disp, boxes, n_boxes, Q, ...); boxes, n_boxes, the rows beyond
    n_boxes and the stream as for box_positions."""
    import torch
    spec = box_spec(select, disparity, band)
    disp, _ = _disparity_batch(disp, "disp")
    B, H, W = disp.shape
    q, xr, xt = _reproject_pointers(Q, XR, XT)
    bx, nb, pos, stat = _box_buffers(boxes, n_boxes, B, disp.device)
    with torch.cuda.device(disp.device):
        rc = box_lib().sv_box_positions_disparity_device(disp.data_ptr(), B, W, H, q, xr, xt, bx.data_ptr(), _ptr(nb), bx.shape[1], ctypes.byref(spec),
                                                         pos.data_ptr(), stat.data_ptr(), torch.cuda.current_stream(disp.device).cuda_stream)
    _check(rc, "sv_box_positions_disparity_device")
    return pos, stat


def cloud_lib():
    """The library with the sv_cloud_* signatures declared."""
    return _bind("cloud")


def cloud_tile():
    """Visited pixels per tile of the compact-cloud kernels (sv_cloud_tile): the unit they count and write by."""
    return int(cloud_lib().sv_cloud_tile())


def cloud_spec(lo=None, hi=None, step=1, disparity="d1", dtype="f32"):
    """-> SvCloudSpec; ValueError for a bad argument (the checks of the C entry, made in Python first)."""
    from .stereo_vision.sv import CLOUD_DISPARITY, CLOUD_DTYPES, cloud_crop
    lo, hi = cloud_crop(lo, hi, step, disparity, dtype)
    spec = SvCloudSpec()
    spec.lo[:] = lo.tolist()
    spec.hi[:] = hi.tolist()
    spec.disparity, spec.step, spec.dtype = CLOUD_DISPARITY[disparity], int(step), CLOUD_DTYPES[dtype]
    return spec


def compact_cloud_from_disparity(d1, Q, colors=None, XR=None, XT=None, lo=None, hi=None, step=1, disparity="d1", dtype="f32", capacity=None,
                                 want_index=False):
    """Compact coloured point clouds straight from disparity maps (CUDA float32 [B,H,W]; one frame [H,W] accepted): per frame the points
    of the visited pixels (every step-th column and row) that carry a disparity and lie strictly inside the crop lo < P < hi (None =
    open; inf / NaN never pass), in pixel order, each point reproject()'s, computed in registers - no dense cloud is written.  disparity
    "dmap": the driver's saturate(round(4 d)) reprojected (a quarter of metric depth), candidates where it is > 0; "d1": d itself
    (metres), candidates where d > 0.  colors: CUDA uint8 [B,H,W,4] (e.g. rig.frontend(..., colors=True)'s) or None; the C entry wants
    them 4-byte aligned (SV_ERR_ARG otherwise), so a view that starts at an odd storage offset is copied first.
    Returns (xyz [B,capacity,3] float32 or float64 ("f64"), color uint8 [B,capacity,4] or None, index int32 [B,capacity] = y * W + x or
    None (want_index), counts int32 [B]): frame b's first min(counts[b], capacity) rows equal stereo_vision.sv.compact_cloud's; counts is
    not capped by the capacity; rows at and beyond counts[b] are undefined.  capacity None = the number of visited pixels, which cannot
    overflow.  CUDA tensors on the input's device, enqueued on torch's current stream (not waited for); split_clouds cuts them."""
    import torch
    spec = cloud_spec(lo, hi, step, disparity, dtype)
    d1, _ = _disparity_batch(d1, "d1")
    B, H, W = d1.shape
    colors = _colors_batch(colors, d1)
    n_visited = -(-W // int(step)) * -(-H // int(step))
    if capacity is None:
        capacity = n_visited
    if isinstance(capacity, bool) or int(capacity) != capacity or not 0 <= capacity < 2 ** 31:
        raise ValueError("capacity must be an integer >= 0, got %r" % (capacity,))
    capacity = int(capacity)
    q, xr, xt = _reproject_pointers(Q, XR, XT)
    dev = d1.device
    xyz = torch.empty((B, capacity, 3), dtype=torch.float32 if dtype == "f32" else torch.float64, device=dev)
    color = torch.empty((B, capacity, 4), dtype=torch.uint8, device=dev) if colors is not None else None
    index = torch.empty((B, capacity), dtype=torch.int32, device=dev) if want_index else None
    counts = torch.empty((B,), dtype=torch.int32, device=dev)  # the scan kernel writes every entry
    if B == 0:  # nothing to enqueue
        return xyz, color, index, counts
    L = cloud_lib()
    nbytes = L.sv_cloud_workspace_bytes(ctypes.byref(spec), B, W, H)
    ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.int32, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        rc = L.sv_cloud_disparity_device(d1.data_ptr(), _ptr(colors), B, W, H, q, xr, xt, ctypes.byref(spec), capacity, _ptr(xyz), _ptr(color), _ptr(index),
                                         counts.data_ptr(), _ptr(ws), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_cloud_disparity_device")
    return xyz, color, index, counts


def split_clouds(xyz, counts, *others):
    """Per-frame views of compact_cloud_from_disparity's padded tensors, cut at min(counts[b], capacity): a list with one xyz[b, :n] per
    frame or, with others (color, index, ...; None entries stay None), one tuple per frame.  Reads counts on the host: the one place that
    synchronises."""
    n = counts.cpu().tolist()
    cap = xyz.shape[1]
    out = []
    for b in range(xyz.shape[0]):
        k = min(int(n[b]), cap)
        out.append(xyz[b, :k] if not others else (xyz[b, :k],) + tuple(None if o is None else o[b, :k] for o in others))
    return out


def voxel_lib():
    """The library with the sv_voxel_* signatures declared."""
    return _bind("voxel")


def voxel_spec(size, lo, hi, step=1, disparity="d1", dtype="f32", capacity=None):
    """-> SvVoxelSpec; ValueError for a bad argument (the checks of the C entry, made in Python first)."""
    from .stereo_vision.sv import CLOUD_DISPARITY, CLOUD_DTYPES, voxel_grid
    lo, hi, size, _ = voxel_grid(size, lo, hi, step, disparity, dtype, capacity)
    spec = SvVoxelSpec()
    spec.lo[:] = lo.tolist()
    spec.hi[:] = hi.tolist()
    spec.size, spec.disparity, spec.step, spec.dtype = size, CLOUD_DISPARITY[disparity], int(step), CLOUD_DTYPES[dtype]
    return spec


def voxel_cloud_from_disparity(d1, Q, size, lo, hi, colors=None, XR=None, XT=None, step=1, disparity="d1", dtype="f32", capacity=None,
                               want_cell=False, want_n=True, want_first=False):
    """Voxel-grid downsampled clouds straight from disparity maps (CUDA float32 [B,H,W]; one frame [H,W] accepted): the points
    compact_cloud_from_disparity would list (same d1, Q, XR / XT, step, disparity; the crop lo < P < hi must be finite), gathered per
    cubic cell of edge `size`: one row per occupied cell with its centroid, the mean colour and the number of points, in the order a
    scan of the image meets the cells.  Neither a dense cloud nor the list of points is written.  colors: CUDA uint8 [B,H,W,4] or None.
    Returns (xyz [B,capacity,3] float32 or float64 ("f64"), color uint8 [B,capacity,4] or None, cell int32 [B,capacity,3] or None
    (want_cell), n int32 [B,capacity] or None (want_n), first int32 [B,capacity] = the smallest y * W + x of the voxel or None
    (want_first), counts int32 [B]): frame b's first counts[b] rows equal stereo_vision.sv.voxel_cloud's, bit for bit; counts[b] is -1
    for a frame with more voxels than `capacity` (its rows mean nothing: raise the capacity); rows at and beyond counts[b] are
    undefined.  capacity None = the number of visited pixels (at most 2^26), which cannot overflow - but the workspace holds a table of
    sv_voxel_table_slots(capacity) entries of 72 bytes PER PAIR, 75 MB for a 1242 x 375 map, and every call clears it: a caller with
    a batch passes a capacity a little above the voxels a frame can have.  CUDA tensors on the input's device, enqueued on torch's
    current stream (not waited for); split_voxel_clouds cuts them."""
    import torch
    spec = voxel_spec(size, lo, hi, step, disparity, dtype, capacity)
    d1, _ = _disparity_batch(d1, "d1")
    B, H, W = d1.shape
    colors = _colors_batch(colors, d1)
    if capacity is None:
        capacity = min(-(-W // int(step)) * -(-H // int(step)), 2 ** 26)
    capacity = int(capacity)
    q, xr, xt = _reproject_pointers(Q, XR, XT)
    dev = d1.device
    xyz = torch.empty((B, capacity, 3), dtype=torch.float32 if dtype == "f32" else torch.float64, device=dev)
    color = torch.empty((B, capacity, 4), dtype=torch.uint8, device=dev) if colors is not None else None
    cell = torch.empty((B, capacity, 3), dtype=torch.int32, device=dev) if want_cell else None
    n = torch.empty((B, capacity), dtype=torch.int32, device=dev) if want_n else None
    first = torch.empty((B, capacity), dtype=torch.int32, device=dev) if want_first else None
    counts = torch.empty((B,), dtype=torch.int32, device=dev)  # the scan kernel writes every entry
    if B == 0:  # nothing to enqueue
        return xyz, color, cell, n, first, counts
    L = voxel_lib()
    nbytes = L.sv_voxel_workspace_bytes(ctypes.byref(spec), B, W, H, capacity)
    if nbytes == ctypes.c_size_t(-1).value:
        raise ValueError("sv_voxel_workspace_bytes refused the request")
    ws = torch.empty(((nbytes + 15) // 16, 2), dtype=torch.int64, device=dev)  # torch's allocations start on 512 bytes
    with torch.cuda.device(dev):
        rc = L.sv_voxel_disparity_device(d1.data_ptr(), _ptr(colors), B, W, H, q, xr, xt, ctypes.byref(spec), capacity, xyz.data_ptr(), _ptr(color), _ptr(cell),
                                         _ptr(n), _ptr(first), counts.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_disparity_device")
    return xyz, color, cell, n, first, counts


def split_voxel_clouds(xyz, counts, *others):
    """split_clouds for voxel_cloud_from_disparity's padded tensors: per-frame views cut at counts[b].  Raises StereoError for a frame
    whose count is -1 (more voxels than the capacity: its rows mean nothing).  Reads counts on the host: the one place that synchronises."""
    over = [b for b, k in enumerate(counts.cpu().tolist()) if k < 0]
    if over:
        raise StereoError("frames %s hold more voxels than the capacity of %d rows: raise the capacity" % (over, xyz.shape[1]))
    return split_clouds(xyz, counts, *others)


def debug_voxel(combine=True, counters=None):
    """sv_debug_voxel: the wavefront merge of the insert kernel on / off and a CUDA int64 [2] tensor (or None) that receives the table
    updates and the atomic instructions issued.  Process-wide; a test hook."""
    return int(voxel_lib().sv_debug_voxel(1 if combine else 0, None if counters is None else counters.data_ptr()))


def ground_lib():
    """The library with the sv_ground_* signatures declared."""
    return _bind("ground")


def ground_spec(height, disp_max=None, n_bins=None, vh_lo=0, vh_hi=None, vh_step=2, qb_step=2, tol=2, g_tol=4, min_run=8, min_support=0):
    """-> SvGroundSpec for maps of `height` rows; ValueError for a bad argument (the checks of the C entry, made in Python first:
    stereo_vision.sv.ground_params).  n_bins None = 4 (disp_max + 1); vh_hi None = height - 2."""
    from .stereo_vision.sv import ground_params
    p = ground_params(height, disp_max, n_bins=n_bins, vh_lo=vh_lo, vh_hi=vh_hi, vh_step=vh_step, qb_step=qb_step, tol=tol, g_tol=g_tol, min_run=min_run,
                      min_support=min_support)
    spec = SvGroundSpec()
    for k, v in p.items():
        setattr(spec, k, v)
    return spec


class GroundResult(_Result):
    """What ground_from_disparity returns, tensors on the input's device: ground int32 [B,4] = (vh, qb, S, n_valid) per pair ((-1, -1, S,
    n_valid): no ground), vdisp uint32-valued int32 [B,H,n_bins], labels uint8 [B,H,W] (0 invalid, 1 ground, 2 obstacle, 3 below the
    ground), free_row int32 [B,W] and free_disp float32 [B,W] (-1 / 0: no obstacle in the column) - None where not asked for - and the
    spec in use.  StereoRig.ground adds pose (per pair (height_m, pitch_rad, slope_px_per_row) or None) and points (float64 [B,W,3]
    numpy, NaN where free_row < 0), both on the host."""
    __slots__ = ("ground", "vdisp", "labels", "free_row", "free_disp", "spec", "pose", "points")


def ground_from_disparity(disp, disp_max=None, n_bins=None, vh_lo=0, vh_hi=None, vh_step=2, qb_step=2, tol=2, g_tol=4, min_run=8, min_support=None,
                          want_vdisp=True, want_labels=True, want_free=True):
    """Ground plane, obstacle labels and free space straight from disparity maps (CUDA float32 [B,H,W]; one frame [H,W] accepted), the
    definition of stereo_vision.sv.ground on the GPU, bit for bit: the v-disparity histogram in quarter-pixel bins
    (n_bins = 4 (disp_max + 1) unless given), the line through (row vh, bin 0) and (row H - 1, bin qb) with the largest support S within
    tol bins - exhaustively over vh = vh_lo .. vh_hi (None = H - 2) in steps of vh_step and qb in steps of qb_step -, a label per
    pixel within / above / below g_tol bins of that line, and per column the lowest row at which min_run obstacle rows begin.
    min_support None = the width: a line with less support is "no ground".  -> GroundResult; enqueued on torch's current stream, not
    waited for."""
    import torch
    d, _ = _disparity_batch(disp, "disp")
    B, H, W = d.shape
    spec = ground_spec(H, disp_max, n_bins, vh_lo, vh_hi, vh_step, qb_step, tol, g_tol, min_run, W if min_support is None else min_support)
    dev = d.device
    ground = torch.empty((B, 4), dtype=torch.int32, device=dev)
    vdisp = torch.empty((B, H, spec.n_bins), dtype=torch.int32, device=dev) if want_vdisp else None
    labels = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_labels else None
    free_row = torch.empty((B, W), dtype=torch.int32, device=dev) if want_free else None
    free_disp = torch.empty((B, W), dtype=torch.float32, device=dev) if want_free else None
    res = GroundResult(ground=ground, vdisp=vdisp, labels=labels, free_row=free_row, free_disp=free_disp, spec=spec)
    if B == 0:  # nothing to enqueue
        return res
    L = ground_lib()
    nbytes = L.sv_ground_workspace_bytes(ctypes.byref(spec), B, W, H)
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.sv_ground_disparity_device(d.data_ptr(), B, W, H, ctypes.byref(spec), _ptr(vdisp), ground.data_ptr(), _ptr(labels), _ptr(free_row),
                                          _ptr(free_disp), ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_ground_disparity_device")
    return res


def stixel_lib():
    """The library with the sv_stixel_* signatures declared."""
    return _bind("stixel")


def stixel_spec(disp_max=None, n_bins=None, q_min=16, sim=6, max_gap=2, min_rows=8, max_layers=8, col_step=1, sim_cols=8, min_cols=16):
    """-> SvStixelSpec; ValueError for a bad argument (the checks of the C entry, made in Python first:
    stereo_vision.sv.stixel_params).  n_bins None = 4 (disp_max + 1), the bins ground_from_disparity uses for the same disp_max."""
    from .stereo_vision.sv import stixel_params
    p = stixel_params(disp_max, n_bins=n_bins, q_min=q_min, sim=sim, max_gap=max_gap, min_rows=min_rows, max_layers=max_layers, col_step=col_step,
                      sim_cols=sim_cols, min_cols=min_cols)
    spec = SvStixelSpec()
    for k, v in p.items():
        setattr(spec, k, v)
    return spec


class StixelResult(_Result):
    """What stixels_from_disparity returns, tensors on the input's device, Wv = ceil(W / col_step) visited columns: stixels int32
    [B,max_layers,Wv,4] = (v_bottom, v_top, q_base, n_rows) per column and layer, bottom-up, -1 beyond a column's count; n_stixels int32
    [B,Wv], not capped; boxes int32 [B,capacity,4] = (x, y, w, h) and info int32 [B,capacity,4] = (n_cols, q_lo, q_hi, q_med) per object,
    left to right, 0 in the rows at and beyond counts[b]; counts int32 [B], not capped by the capacity - None where not asked for - and
    the spec in use.  StereoRig.objects adds positions (float64 [B,capacity,3] metres, NaN beyond counts) and ground (a GroundResult)."""
    __slots__ = ("stixels", "n_stixels", "boxes", "info", "counts", "spec", "positions", "stat", "ground")


def stixels_from_disparity(d1, labels, disp_max=None, n_bins=None, q_min=16, sim=6, max_gap=2, min_rows=8, max_layers=8, col_step=1, sim_cols=8,
                           min_cols=16, capacity=64, want_stixels=True, want_objects=True):
    """The stixel world and detector-free object boxes of disparity maps (CUDA float32 [B,H,W]; one frame [H,W] accepted) and their
    obstacle labels (CUDA uint8, the same shape: ground_from_disparity's), the definition of stereo_vision.sv.stixels and
    stixel_objects on the GPU, bit for bit.  Per visited column (every col_step-th) the runs of foreground rows - label 2, d > 0, bin
    >= q_min - within sim bins of the run's bottom row, bridging up to max_gap rows, of at least min_rows rows; objects are runs of at
    least min_cols visited columns whose first stixels are within sim_cols bins of their left neighbour's.  boxes / counts go straight
    into box_positions_from_disparity(d1, Q, boxes, counts).  n_bins None = 4 (disp_max + 1), as for the labels.  -> StixelResult;
    enqueued on torch's current stream, not waited for."""
    import torch
    d, _ = _disparity_batch(d1, "d1", 32768)
    if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.uint8 and labels.device == d1.device and
            tuple(labels.shape) == tuple(d1.shape)):
        raise ValueError("labels must be a CUDA uint8 tensor of d1's shape on d1's device")
    lab = (labels.unsqueeze(0) if labels.dim() == 2 else labels).contiguous()
    B, H, W = d.shape
    if isinstance(capacity, bool) or int(capacity) != capacity or not 0 <= capacity < 2 ** 31:
        raise ValueError("capacity must be an integer >= 0, got %r" % (capacity,))
    capacity = int(capacity)
    spec = stixel_spec(disp_max, n_bins, q_min, sim, max_gap, min_rows, max_layers, col_step, sim_cols, min_cols)
    dev = d.device
    Wv = -(-W // spec.col_step)
    stixels = torch.empty((B, spec.max_layers, Wv, 4), dtype=torch.int32, device=dev) if want_stixels else None
    n_stixels = torch.empty((B, Wv), dtype=torch.int32, device=dev) if want_stixels else None
    boxes = torch.zeros((B, capacity, 4), dtype=torch.int32, device=dev) if want_objects else None  # the rows beyond counts are not written
    info = torch.zeros((B, capacity, 4), dtype=torch.int32, device=dev) if want_objects else None
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    res = StixelResult(stixels=stixels, n_stixels=n_stixels, boxes=boxes, info=info, counts=counts, spec=spec)
    if B == 0:  # nothing to enqueue
        return res
    L = stixel_lib()
    nbytes = L.sv_stixel_workspace_bytes(ctypes.byref(spec), B, W, H)
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.sv_stixel_disparity_device(d.data_ptr(), lab.data_ptr(), B, W, H, ctypes.byref(spec), capacity, _ptr(stixels), _ptr(n_stixels), _ptr(boxes),
                                          _ptr(info), counts.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_stixel_disparity_device")
    return res


def occupancy_lib():
    """The library with the sv_occupancy_* signatures declared."""
    return _bind("occupancy")


def occupancy_spec(x_range, y_range, z_range, scale, z_scale=20, min_obstacle=3, min_ground=1, min_rays=1, XT=None):
    """-> (SvOccupancySpec, rows, cols); ValueError for a bad argument (the checks of the C entry, made in Python first:
    stereo_vision.sv.occupancy_params)."""
    from .stereo_vision.sv import occupancy_params
    rows, cols, p = occupancy_params(x_range, y_range, z_range, scale, z_scale, min_obstacle, min_ground, min_rays, XT)
    spec = SvOccupancySpec()
    spec.x_range[:] = [float(v) for v in x_range]
    spec.y_range[:] = [float(v) for v in y_range]
    spec.z_range[:] = [float(v) for v in z_range]
    spec.scale = int(scale)
    for k, v in p.items():
        setattr(spec, k, v)
    return spec, rows, cols


class OccupancyResult(_Result):
    """What occupancy_from_disparity returns, tensors on the input's device: cells int32 [B,rows,cols,4] = (n_ground, n_obstacle, h_lo,
    h_hi) per cell (h in steps of 1 / z_scale above z_range[0], -1 for a cell without evidence: stereo_vision.sv.occupancy_heights turns
    them into metres), n_rays int32 [B,rows,cols] = the sight lines that crossed the cell, state uint8 [B,rows,cols] (0 unknown, 1 free,
    2 occupied; None where not asked for) and the spec in use.  StereoRig.occupancy adds ground, the GroundResult the grid was made
    from."""
    __slots__ = ("cells", "n_rays", "state", "spec", "ground")


def occupancy_from_disparity(d1, labels, free_row, free_disp, Q, x_range, y_range, z_range, scale, z_scale=20, XR=None, XT=None, min_obstacle=3,
                             min_ground=1, min_rays=1, want_state=True):
    """Occupancy and elevation grids straight from disparity maps (CUDA float32 [B,H,W]; one frame [H,W] accepted), their labels (uint8
    [B,H,W]) and free space (free_row int32 [B,W], free_disp float32 [B,W]) as ground_from_disparity returns them - the definition of
    stereo_vision.sv.occupancy_grid on the GPU, bit for bit.  The grid is top_view's (x_range, y_range, z_range, scale, mode "count") in
    the frame XR P + XT of the "d1" points, metres.  Per cell: the ground and obstacle pixels that fell into it, the lowest and highest
    height step (z_scale per metre above z_range[0]) of either, the sight lines - one per image column, from the camera centre to the
    column's obstacle base or else its topmost ground pixel - that crossed it, and a state: 2 occupied (n_obstacle >= min_obstacle), else
    1 free (n_ground >= min_ground or n_rays >= min_rays), else 0 unknown.  Nothing dense is read back and no cloud is written.
    -> OccupancyResult; enqueued on torch's current stream, not waited for."""
    import torch
    spec, rows, cols = occupancy_spec(x_range, y_range, z_range, scale, z_scale, min_obstacle, min_ground, min_rays, XT)
    d, one = _disparity_batch(d1, "d1", 32768)
    B, H, W = d.shape
    dev = d.device
    ins = []
    for t, dtype, shape, name in ((labels, torch.uint8, (B, H, W), "labels"), (free_row, torch.int32, (B, W), "free_row"), (free_disp, torch.float32, (B, W), "free_disp")):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype):
            raise ValueError("%s must be a %s tensor on the device of d1" % (name, dtype))
        t = t.unsqueeze(0) if one and t.dim() == len(shape) - 1 else t
        if tuple(t.shape) != shape:
            raise ValueError("%s must be %s, got %s" % (name, list(shape), list(t.shape)))
        ins.append(t.contiguous())
    q, xr, xt = _reproject_pointers(Q, XR, XT)
    cells = torch.empty((B, rows, cols, 4), dtype=torch.int32, device=dev)
    n_rays = torch.empty((B, rows, cols), dtype=torch.int32, device=dev)
    state = torch.empty((B, rows, cols), dtype=torch.uint8, device=dev) if want_state else None
    res = OccupancyResult(cells=cells, n_rays=n_rays, state=state, spec=spec)
    if B == 0:  # nothing to enqueue
        return res
    L = occupancy_lib()
    with torch.cuda.device(dev):
        rc = L.sv_occupancy_disparity_device(d.data_ptr(), ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), B, W, H, q, xr, xt,
                                             ctypes.byref(spec), cells.data_ptr(), n_rays.data_ptr(), _ptr(state), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_occupancy_disparity_device")
    return res


def debug_occupancy(combine=True, counter=None):
    """sv_debug_occupancy: the wavefront merge of the evidence kernel on / off and a CUDA int64 [1] tensor (or None) that receives the
    atomics issued on the cells.  Process-wide; a test hook."""
    return int(occupancy_lib().sv_debug_occupancy(1 if combine else 0, None if counter is None else counter.data_ptr()))


def occupancy_map_lib():
    """The library with the signatures of group (K) declared."""
    return _bind("occupancy_map")


def _occupancy_map_struct(words):
    spec = SvOccupancyMapSpec()
    for k, v in words.items():
        setattr(spec, k, v)
    return spec


def occupancy_map_spec(x_range, y_range, scale, l_occ=85, l_free=40, l_min=-200, l_max=350):
    """-> SvOccupancyMapSpec of the world map over x_range x y_range at `scale` uniform cells per metre; ValueError for a bad argument
    (the checks of the C entry, made in Python first: stereo_vision.sv.occupancy_map_params)."""
    from .stereo_vision.sv import occupancy_map_params
    return _occupancy_map_struct(occupancy_map_params(x_range, y_range, scale, l_occ, l_free, l_min, l_max))


def _occupancy_frame_spec(frame_grid):
    """-> SvOccupancySpec of a frame grid given as one, or as a dict of occupancy_spec's arguments (z_range may be left out)."""
    from .stereo_vision.sv import occupancy_frame_grid
    occupancy_frame_grid(frame_grid)  # argument errors
    if isinstance(frame_grid, SvOccupancySpec):
        return frame_grid
    g = dict(frame_grid) if isinstance(frame_grid, dict) else {k: getattr(frame_grid, k) for k in ("x_range", "y_range", "z_range", "scale") if hasattr(frame_grid, k)}
    keys = ("x_range", "y_range", "z_range", "scale", "z_scale", "min_obstacle", "min_ground", "min_rays")
    g = {k: (tuple(v) if k.endswith("_range") else v) for k, v in g.items() if k in keys}
    g.setdefault("z_range", (0, 1))
    return occupancy_spec(**g)[0]


def _state_batch(L, state, frame):
    """The states of a batch of frames, checked against the frame grid they were made under -> the contiguous CUDA uint8 tensor [B,frame
    rows,frame cols] (one frame gets its B here)."""
    import torch
    frows, fcols = ctypes.c_int(), ctypes.c_int()
    _check(L.sv_occupancy_dims(ctypes.byref(frame), ctypes.byref(frows), ctypes.byref(fcols)), "sv_occupancy_dims")
    if not (isinstance(state, torch.Tensor) and state.is_cuda and state.dtype == torch.uint8 and state.dim() in (2, 3)):
        raise ValueError("state must be a CUDA uint8 tensor [B,rows,cols]")
    st = (state.unsqueeze(0) if state.dim() == 2 else state).contiguous()
    if tuple(st.shape[1:]) != (frows.value, fcols.value):
        raise ValueError("state must be [B,%d,%d] for this frame grid, got %s" % (frows.value, fcols.value, tuple(st.shape)))
    return st


def _device_poses(poses, dev):
    """Poses (tx, ty, c, s) as a contiguous float64 tensor on dev: a tensor there as it is, a numpy array uploaded once."""
    import torch
    if isinstance(poses, torch.Tensor):
        if poses.device != dev or poses.dtype != torch.float64:
            raise ValueError("poses must be float64 on the device (%s) of the other tensors" % (dev,))
        return poses.contiguous()
    return torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).to(dev)


class OccupancyMapResult(_Result):
    """What occupancy_fuse returns: logodds int16 [rows,cols], last_seen int32 [rows,cols] (None where none is kept) - tensors on the
    states' device - and spec, the SvOccupancyMapSpec of the map going out."""
    __slots__ = ("logodds", "last_seen", "spec")


def occupancy_fuse(state, poses, frame_grid, map, logodds=None, last_seen=None, seq0=0, shift=(0, 0), out=None):
    """The states of B frames (uint8 [B,frame rows,frame cols], e.g. OccupancyResult.state; one frame without B accepted) fused along
    their poses (float64 [B,4] = (tx, ty, c, s): stereo_vision.sv.occupancy_pose; a numpy array - uploaded once - or a tensor on the
    states' device) into a world-fixed log-odds map - the definition of stereo_vision.sv.occupancy_fuse on the GPU, bit for bit, in one
    kernel that reads the map once and writes it once.  frame_grid: the SvOccupancySpec the states were made under (OccupancyResult.spec)
    or a dict of x_range, y_range, scale.  map: an SvOccupancyMapSpec (occupancy_map_spec) or a dict of its nine words, describing the
    map going out; with shift = (rows, cols) != (0, 0) the map scrolls by whole cells - the map coming in, whose top and left were
    top + shift[0] and left + shift[1], is read at (r + shift[0], c + shift[1]), 0 / -1 outside.  logodds / last_seen: the map coming in (None: a fresh map;
    last_seen=False: none is kept).  Without a shift the map is updated in place; with one, into `out` = (logodds, last_seen) or into
    new tensors.  Frame b carries the sequence number seq0 + b into last_seen.  -> OccupancyMapResult; enqueued on torch's current
    stream, not waited for."""
    import torch
    from .stereo_vision.sv import occupancy_map_words
    words = occupancy_map_words(map)
    rows, cols = words["rows"], words["cols"]
    frame = _occupancy_frame_spec(frame_grid)
    L = occupancy_map_lib()
    st = _state_batch(L, state, frame)
    B, dev = st.shape[0], st.device
    if B > 65535:
        raise ValueError("at most 65535 frames per call, got %d" % B)
    if isinstance(seq0, bool) or int(seq0) != seq0 or seq0 < 0 or int(seq0) + B > 2 ** 31 - 1:
        raise ValueError("seq0 must be an integer >= 0 with seq0 + B below 2^31, got %r" % (seq0,))
    if len(shift) != 2 or any(isinstance(v, bool) or int(v) != v or abs(int(v)) > 2 ** 31 - 1 for v in shift):
        raise ValueError("shift must be two integers (rows, cols), got %r" % (shift,))
    shift = (int(shift[0]), int(shift[1]))
    p = _device_poses(poses, dev)
    if p.dim() == 1 and B == 1:
        p = p.unsqueeze(0)
    if tuple(p.shape) != (B, 4):
        raise ValueError("poses must be [%d,4], got %s" % (B, tuple(p.shape)))
    keep_seen = last_seen is not False

    def given(t, dtype, name):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == (rows, cols) and t.is_contiguous()):
            raise ValueError("%s must be a contiguous %s tensor [%d,%d] on the device of state" % (name, dtype, rows, cols))
        return t

    l_in = torch.zeros((rows, cols), dtype=torch.int16, device=dev) if logodds is None else given(logodds, torch.int16, "logodds")
    s_in = None
    if keep_seen:
        s_in = torch.full((rows, cols), -1, dtype=torch.int32, device=dev) if last_seen is None else given(last_seen, torch.int32, "last_seen")
    if out is not None:
        l_out = given(out[0], torch.int16, "out[0]")
        s_out = given(out[1], torch.int32, "out[1]") if keep_seen else None
    elif shift == (0, 0):
        l_out, s_out = l_in, s_in
    else:
        l_out, s_out = torch.empty_like(l_in), (torch.empty_like(s_in) if keep_seen else None)
    spec = _occupancy_map_struct(words)
    with torch.cuda.device(dev):
        rc = L.sv_occupancy_fuse_device(_ptr(st), _ptr(p), B, int(seq0), ctypes.byref(frame), ctypes.byref(spec), shift[0], shift[1], l_in.data_ptr(), _ptr(s_in),
                                        l_out.data_ptr(), _ptr(s_out), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_occupancy_fuse_device")
    return OccupancyMapResult(logodds=l_out, last_seen=s_out, spec=spec)


def debug_occupancy_fuse(cull=True, counter=None):
    """sv_debug_occupancy_fuse: the per-wavefront cull of frames on / off and a CUDA int64 [1] tensor (or None) that receives the per-lane
    lookups made.  Process-wide; a test hook."""
    return int(occupancy_map_lib().sv_debug_occupancy_fuse(1 if cull else 0, None if counter is None else counter.data_ptr()))


def map_match_lib():
    """The library with the signatures of group (L) declared."""
    return _bind("map_match")


class MapMatchResult(_Result):
    """What occupancy_match returns, tensors on the states' device: sums int64 [B,P,2] = (H, M), counts int32 [B,P,2] = (n_occ, n_free)
    (both None where not asked for), best int32 [B] and best_score int64 [B] (both None where not asked for)."""
    __slots__ = ("sums", "counts", "best", "best_score")

    def score(self, w_occ=1, w_free=0):
        """int64 [B,P]: w_occ H - w_free M of the sums."""
        return w_occ * self.sums[..., 0] - w_free * self.sums[..., 1]


def occupancy_match(state, poses, frame_grid, map, logodds, w_occ=1, w_free=0, want_sums=True, want_best=True):
    """The states of B frames (CUDA uint8 [B,frame rows,frame cols], e.g. OccupancyResult.state; one frame without B accepted) scored
    against a world map's logodds (int16 [rows,cols] on the same device, e.g. OccupancyMapResult.logodds) at P candidate poses per frame
    (float64 [B,P,4] = (tx, ty, c, s): stereo_vision.sv.occupancy_pose of occupancy_pose_window's rows; a numpy array - uploaded once -
    or a tensor on the states' device; [P,4] accepted for one frame) - the definition of stereo_vision.sv.occupancy_match on the GPU, bit
    for bit: per candidate the sum of the map's log-odds under the frame's occupied cells (and, with w_free > 0, under its free cells) and
    how many landed in the map, and per frame the lowest candidate with the largest score w_occ H - w_free M.  frame_grid and map as for
    occupancy_fuse.  Nothing dense is read back; the workspace comes from torch.  -> MapMatchResult; enqueued on torch's current stream,
    not waited for."""
    import torch
    from .stereo_vision.sv import occupancy_map_words
    words = occupancy_map_words(map)
    rows, cols = words["rows"], words["cols"]
    frame = _occupancy_frame_spec(frame_grid)
    L = map_match_lib()
    st = _state_batch(L, state, frame)
    B, dev = st.shape[0], st.device
    p = _device_poses(poses, dev)
    if p.dim() == 2 and B == 1:
        p = p.unsqueeze(0)
    if p.dim() != 3 or p.shape[0] != B or p.shape[2] != 4:
        raise ValueError("poses must be [%d,P,4], got %s" % (B, tuple(p.shape)))
    n_poses = p.shape[1]
    if B > 65535 or not 1 <= n_poses <= 65535 or B * n_poses >= 2 ** 31:
        raise ValueError("at most 65535 frames of 1 .. 65535 poses each and fewer than 2^31 in all, got %d x %d" % (B, n_poses))
    for v in (w_occ, w_free):
        if isinstance(v, bool) or int(v) != v or not 0 <= v <= 32767:
            raise ValueError("w_occ and w_free must be integers in 0 .. 32767, got %r, %r" % (w_occ, w_free))
    if int(w_occ) == 0 and int(w_free) == 0:
        raise ValueError("w_occ and w_free must not both be 0")
    if not (want_sums or want_best):
        raise ValueError("neither the sums nor the best are asked for")
    if not (isinstance(logodds, torch.Tensor) and logodds.device == dev and logodds.dtype == torch.int16 and tuple(logodds.shape) == (rows, cols) and logodds.is_contiguous()):
        raise ValueError("logodds must be a contiguous int16 tensor [%d,%d] on the device of state" % (rows, cols))
    res = MapMatchResult()
    if want_sums:
        res.sums = torch.empty((B, n_poses, 2), dtype=torch.int64, device=dev)
        res.counts = torch.empty((B, n_poses, 2), dtype=torch.int32, device=dev)
    if want_best:
        res.best = torch.empty((B,), dtype=torch.int32, device=dev)
        res.best_score = torch.empty((B,), dtype=torch.int64, device=dev)
    if B == 0:  # nothing to enqueue
        return res
    nbytes = ctypes.c_size_t()
    _check(L.sv_map_match_workspace(ctypes.byref(frame), B, int(w_free), ctypes.byref(nbytes)), "sv_map_match_workspace")
    ws = torch.empty((nbytes.value + 15) // 16 * 2, dtype=torch.int64, device=dev)
    spec = _occupancy_map_struct(words)
    with torch.cuda.device(dev):
        rc = L.sv_map_match_device(st.data_ptr(), p.data_ptr(), B, n_poses, ctypes.byref(frame), ctypes.byref(spec), logodds.data_ptr(), int(w_occ), int(w_free),
                                   _ptr(res.sums), _ptr(res.counts), _ptr(res.best), _ptr(res.best_score), ws.data_ptr(), ws.numel() * 8,
                                   torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_map_match_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def debug_map_match(group=0, counter=None):
    """sv_debug_map_match: the candidates a workgroup scores (0: the call chooses; a power of two in 1 .. 256) and a CUDA int64 [1] tensor
    (or None) that receives the map lookups made.  Process-wide; a test hook."""
    return int(map_match_lib().sv_debug_map_match(int(group), None if counter is None else counter.data_ptr()))


def clearance_lib():
    """The library with the signatures of group (M) declared."""
    return _bind("clearance")


def occupancy_clearance(logodds, radius, t_occ, last_seen=None, unknown=False, out=None, workspace=None):
    """The clearance field of a world map - the definition of stereo_vision.sv.occupancy_clearance on the GPU, bit for bit, in one fused
    call of two kernels: logodds a contiguous CUDA int16 tensor [rows,cols] (e.g. OccupancyMapResult.logodds), last_seen an int32 tensor
    of the same shape on the same device or None, radius in cells (1 .. 254), t_occ in the int16 range; with unknown, cells never seen
    (last_seen < 0) are sources too.  out: a contiguous uint16 tensor [rows,cols] to write into; workspace: a uint8 tensor of at least
    rows x cols bytes (rounded up to 16) to reuse - both come from torch where not given.  -> the uint16 tensor [rows,cols]: per cell
    the squared distance in cells to the nearest source, 65535 beyond radius; enqueued on torch's current stream, not waited for."""
    import torch
    from .stereo_vision.sv import CLEARANCE_RADIUS_MAX
    if not (isinstance(logodds, torch.Tensor) and logodds.is_cuda and logodds.dtype == torch.int16 and logodds.dim() == 2 and logodds.is_contiguous()):
        raise ValueError("logodds must be a contiguous CUDA int16 tensor [rows,cols]")
    rows, cols = logodds.shape
    dev = logodds.device
    if not (1 <= rows <= 32768 and 1 <= cols <= 32768):
        raise ValueError("a map of %d x %d cells: 1 .. 32768 in either dimension" % (rows, cols))
    for v, lo, hi, what in ((radius, 1, CLEARANCE_RADIUS_MAX, "radius"), (t_occ, -32768, 32767, "t_occ")):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    if not isinstance(unknown, bool) and unknown not in (0, 1):
        raise ValueError("unknown must be 0 or 1, got %r" % (unknown,))
    if unknown and last_seen is None:
        raise ValueError("unknown needs last_seen")
    if last_seen is not None and not (isinstance(last_seen, torch.Tensor) and last_seen.device == dev and last_seen.dtype == torch.int32
                                      and tuple(last_seen.shape) == (rows, cols) and last_seen.is_contiguous()):
        raise ValueError("last_seen must be a contiguous int32 tensor [%d,%d] on the device of logodds" % (rows, cols))
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.uint16, device=dev)
    elif not (isinstance(out, torch.Tensor) and out.device == dev and out.dtype == torch.uint16 and tuple(out.shape) == (rows, cols) and out.is_contiguous()):
        raise ValueError("out must be a contiguous uint16 tensor [%d,%d] on the device of logodds" % (rows, cols))
    L = clearance_lib()
    nbytes = ctypes.c_size_t()
    _check(L.sv_clearance_workspace(rows, cols, ctypes.byref(nbytes)), "sv_clearance_workspace")
    if workspace is None:
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    elif not (isinstance(workspace, torch.Tensor) and workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous()
              and workspace.numel() >= nbytes.value):
        raise ValueError("workspace must be a contiguous uint8 tensor of at least %d bytes on the device of logodds" % nbytes.value)
    with torch.cuda.device(dev):
        rc = L.sv_clearance_device(logodds.data_ptr(), _ptr(last_seen), rows, cols, int(radius), int(t_occ), int(bool(unknown)),
                                   out.data_ptr(), workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_clearance_device")
    return out  # a workspace of torch's goes back to its allocator, which hands it out again on this stream only: behind the kernels


class ClearancePathsResult(_Result):
    """What clearance_paths returns, int32 tensors [K] on the field's device: first_hit (the number of steps where a path is clear),
    min_d2 (65535 where nothing was looked up) and n_outside."""
    __slots__ = ("first_hit", "min_d2", "n_outside")


def clearance_paths(d2, map, poses, discs, radius):
    """K candidate paths checked against a clearance field - the definition of stereo_vision.sv.clearance_paths on the GPU, bit for bit,
    in one kernel: d2 a contiguous CUDA uint16 tensor [rows,cols] (occupancy_clearance's with `radius`), map an SvOccupancyMapSpec or a
    dict of its nine words, poses float64 [K,T,4] = (tx, ty, c, s) (a numpy array - uploaded once - or a tensor on d2's device), discs =
    (centres float64 [n,2], r2 int [n]) as stereo_vision.sv.clearance_discs gives them, every r2 <= radius^2.  -> ClearancePathsResult;
    enqueued on torch's current stream, not waited for; nothing dense is read back."""
    import torch
    from .stereo_vision.sv import CLEARANCE_PATHS_MAX, _clearance_footprint, occupancy_map_words
    words = occupancy_map_words(map)
    rows, cols = words["rows"], words["cols"]
    centres, r2, radius = _clearance_footprint(discs[0], discs[1], radius)
    if not (isinstance(d2, torch.Tensor) and d2.is_cuda and d2.dtype == torch.uint16 and tuple(d2.shape) == (rows, cols) and d2.is_contiguous()):
        raise ValueError("d2 must be a contiguous CUDA uint16 tensor [%d,%d]" % (rows, cols))
    dev = d2.device
    p = _device_poses(poses, dev)
    if p.dim() != 3 or p.shape[2] != 4 or p.shape[0] > CLEARANCE_PATHS_MAX or not 1 <= p.shape[1] <= CLEARANCE_PATHS_MAX:
        raise ValueError("poses must be [K,T,4] with K <= 65535 and 1 <= T <= 65535, got %s" % (tuple(p.shape),))
    K, T = p.shape[:2]
    res = ClearancePathsResult(**{k: torch.empty((K,), dtype=torch.int32, device=dev) for k in ClearancePathsResult.__slots__})
    if K == 0:  # nothing to enqueue
        return res
    spec = _occupancy_map_struct(words)
    L = clearance_lib()
    with torch.cuda.device(dev):
        rc = L.sv_clearance_paths_device(d2.data_ptr(), ctypes.byref(spec), p.data_ptr(), K, T, centres.ctypes.data, r2.ctypes.data, len(r2), radius,
                                         res.first_hit.data_ptr(), res.min_d2.data_ptr(), res.n_outside.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_clearance_paths_device")
    return res


def debug_clearance(variant=0, counter=None):
    """sv_debug_clearance: the kernels of occupancy_clearance (0: the call chooses; 1: both passes in one kernel where radius <= 32; 2: the
    two kernels; 3: the two kernels without the early exit) and a CUDA int64 [1] tensor (or None) that receives the taps of the row walk.
    Process-wide; a test hook."""
    return int(clearance_lib().sv_debug_clearance(int(variant), None if counter is None else counter.data_ptr()))


def cost_lib():
    """The library with the signatures of group (N) declared."""
    return _bind("cost")


def _map_tensor(t, dtype, name, like=None):
    """A field of the world map, checked: a contiguous CUDA tensor [rows,cols] of `dtype`, on the device and of the shape of `like` where
    that is given -> (rows, cols)."""
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.is_contiguous()
            and (like is None or (t.device == like.device and t.shape == like.shape))):
        raise ValueError("%s must be a contiguous CUDA %s tensor [rows,cols]%s" % (name, str(dtype).replace("torch.", ""),
                                                                                 "" if like is None else " %s on %s" % (tuple(like.shape), like.device)))
    rows, cols = t.shape
    if not (1 <= rows <= 32768 and 1 <= cols <= 32768):
        raise ValueError("a map of %d x %d cells: 1 .. 32768 in either dimension" % (rows, cols))
    return rows, cols


def _cell_list(cells, dev, lo, hi, name):
    """Goals or starts -> a contiguous int32 tensor [n,2] on dev: a numpy array or a list is uploaded, a tensor on dev is taken as it is."""
    import torch
    from .stereo_vision.sv import _cost_cell_list
    if isinstance(cells, torch.Tensor):
        if cells.device != dev or cells.dtype != torch.int32 or cells.dim() != 2 or cells.shape[1] != 2 or not lo <= cells.shape[0] <= hi:
            raise ValueError("%s as a tensor must be int32 [n,2] on %s with %d <= n <= %d" % (name, dev, lo, hi))
        return cells.contiguous()
    return torch.from_numpy(_cost_cell_list(cells, lo, hi, name)).to(dev)


def cost_cells(d2, radius, r2_block, soft=0, weight=0, out=None):
    """The penalties of a clearance field - the definition of stereo_vision.sv.cost_cells on the GPU, bit for bit, in one element-wise
    kernel: d2 a contiguous CUDA uint16 tensor [rows,cols] (occupancy_clearance's with `radius`), r2_block in 0 .. radius^2, soft and
    weight in 0 .. 254; out: a contiguous uint8 tensor [rows,cols] to write into.  -> the uint8 tensor: 255 where d2 <= r2_block,
    elsewhere min(254, weight * max(0, soft - isqrt(d2))); enqueued on torch's current stream, not waited for."""
    import torch
    rows, cols = _map_tensor(d2, torch.uint16, "d2")
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.uint8, device=d2.device)
    else:
        _map_tensor(out, torch.uint8, "out", like=d2)
    for v, what in ((radius, "radius"), (r2_block, "r2_block"), (soft, "soft"), (weight, "weight")):
        if isinstance(v, bool) or int(v) != v or abs(v) > 2 ** 31 - 1:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    with torch.cuda.device(d2.device):
        rc = cost_lib().sv_cost_cells_device(d2.data_ptr(), rows, cols, int(radius), int(r2_block), int(soft), int(weight), out.data_ptr(),
                                             torch.cuda.current_stream(d2.device).cuda_stream)
    _check(rc, "sv_cost_cells_device")
    return out


class CostToGoalResult(_Result):
    """What occupancy_cost_to_goal returns: cost (int32 tensor [rows,cols]), converged (bool), sweeps (int: the sweeps that changed a
    cell, and one more for the sweep that confirmed the fixed point where it was reached) and workspace (the uint8 tensor the state of the
    sweeps lives in)."""
    __slots__ = ("cost", "converged", "sweeps", "workspace")


def occupancy_cost_to_goal(pen, goals, max_sweeps=4096, round=16, out=None, workspace=None):
    """The cost-to-goal field of a world map - the definition of stereo_vision.sv.cost_to_goal on the GPU, bit for bit once converged: pen
    a contiguous CUDA uint8 tensor [rows,cols] (cost_cells', or the caller's own; 255 = blocked; rows x cols <= 8 000 000), goals integers
    [G,2] = (row, col), 1 <= G <= 1024 (numpy - uploaded once - or an int32 tensor on pen's device); those outside the map or on blocked
    cells are ignored.  out: a contiguous int32 tensor [rows,cols] to write into; workspace: a uint8 tensor of at least
    sv_cost_to_goal_workspace's bytes to reuse.

    The C entry is called in rounds of `round` sweeps (even, 2 .. 1024; the last round is cut to what max_sweeps leaves, made even) and
    enqueues on torch's current stream without waiting; after each round the 16 bytes of its info are read back - the only wait - and
    the rounds stop once a round's last sweep changed nothing, or after max_sweeps.  -> CostToGoalResult.  With converged == False the
    field is an upper bound of the definition, cell by cell: every finite cost in it is the length of some admissible path, only not
    yet of the cheapest one."""
    import torch
    rows, cols = _map_tensor(pen, torch.uint8, "pen")
    dev = pen.device
    if rows * cols > 8000000:
        raise ValueError("a field of %d x %d cells: at most 8 000 000, so that every cost stays below 2^31 - 1" % (rows, cols))
    for v, lo, hi, what in ((max_sweeps, 1, 2 ** 31 - 1, "max_sweeps"), (round, 2, 1024, "round")):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    if round % 2:
        raise ValueError("round must be even, got %r" % (round,))
    g = _cell_list(goals, dev, 1, 1024, "goals")
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.int32, device=dev)
    else:
        _map_tensor(out, torch.int32, "out", like=pen)
    L = cost_lib()
    nbytes = ctypes.c_size_t()
    _check(L.sv_cost_to_goal_workspace(rows, cols, ctypes.byref(nbytes)), "sv_cost_to_goal_workspace")
    if workspace is None:
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    elif not (isinstance(workspace, torch.Tensor) and workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous()
              and workspace.numel() >= nbytes.value):
        raise ValueError("workspace must be a contiguous uint8 tensor of at least %d bytes on the device of pen" % nbytes.value)
    info = torch.empty(4, dtype=torch.int32, device=dev)
    done, changing, converged = 0, 0, False
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        while done < max_sweeps and not converged:
            n = min(int(round), int(max_sweeps) - done)
            n += n & 1
            rc = L.sv_cost_to_goal_device(pen.data_ptr(), rows, cols, g.data_ptr(), g.shape[0], int(done == 0), n, out.data_ptr(), workspace.data_ptr(),
                                          workspace.numel(), info.data_ptr(), stream)
            _check(rc, "sv_cost_to_goal_device")
            words = info.cpu().numpy()  # 16 bytes: the wait of the round
            done += n
            changing += int(words[1])
            converged = int(words[0]) == 0
    return CostToGoalResult(cost=out, converged=converged, sweeps=changing + int(converged), workspace=workspace)


class CostRoutesResult(_Result):
    """What cost_routes returns, tensors on the field's device: cells int16 [K,capacity,2] = (row, col), -1 past a route's length; length
    int32 [K]; status int32 [K] - 0 a goal was reached, 1 the start is outside the map, 2 it is blocked or no goal reaches it, 3 capacity
    cells were written first, 4 the field was not converged where the route stopped."""
    __slots__ = ("cells", "length", "status")


def cost_routes(cost, pen, starts, capacity):
    """K routes walked down a cost-to-goal field - the definition of stereo_vision.sv.cost_routes on the GPU, bit for bit, in one kernel
    of 8 lanes per route: cost a contiguous CUDA int32 tensor [rows,cols] (occupancy_cost_to_goal's), pen the uint8 tensor it was made
    from, starts integers [K,2] = (row, col), 0 <= K <= 65535 (numpy or an int32 tensor on the device), capacity in 1 .. 65535 cells per
    route.  -> CostRoutesResult; enqueued on torch's current stream, not waited for."""
    import torch
    rows, cols = _map_tensor(cost, torch.int32, "cost")
    _map_tensor(pen, torch.uint8, "pen", like=cost)
    dev = cost.device
    if rows * cols > 8000000:
        raise ValueError("a field of %d x %d cells: at most 8 000 000" % (rows, cols))
    if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= capacity <= 65535:
        raise ValueError("capacity must be an integer in 1 .. 65535, got %r" % (capacity,))
    s = _cell_list(starts, dev, 0, 65535, "starts")
    K = s.shape[0]
    res = CostRoutesResult(cells=torch.empty((K, int(capacity), 2), dtype=torch.int16, device=dev), length=torch.empty((K,), dtype=torch.int32, device=dev),
                           status=torch.empty((K,), dtype=torch.int32, device=dev))
    if K == 0:  # nothing to enqueue
        return res
    with torch.cuda.device(dev):
        rc = cost_lib().sv_cost_routes_device(cost.data_ptr(), pen.data_ptr(), rows, cols, s.data_ptr(), K, int(capacity), res.cells.data_ptr(),
                                              res.length.data_ptr(), res.status.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_cost_routes_device")
    return res


def debug_cost_to_goal(variant=0, counters=None):
    """sv_debug_cost_to_goal: the tiles a sweep of occupancy_cost_to_goal runs (0: those the dirty bytes name; 1: every tile in every
    sweep) and a CUDA int64 [2] tensor (or None) that receives the tiles run and their inner iterations.  Process-wide; a test hook."""
    return int(cost_lib().sv_debug_cost_to_goal(int(variant), None if counters is None else counters.data_ptr()))


def frontier_lib():
    """The library with the signatures of group (O) declared."""
    return _bind("frontier")


def frontier_cells(logodds, last_seen, occupied, free, pen=None, out=None):
    """The frontier cells of a world map - the definition of stereo_vision.sv.frontier_cells on the GPU, bit for bit, in one kernel:
    logodds a contiguous CUDA int16 tensor [rows,cols], last_seen an int32 tensor and pen a uint8 tensor (cost_cells', or None) of the
    same shape on the same device, occupied and free the thresholds of the state; out: a contiguous uint8 tensor [rows,cols] to write
    into.  -> the uint8 tensor: 1 on a free cell that the vehicle can stand on and that touches a cell nobody has decided yet, else 0;
    enqueued on torch's current stream, not waited for."""
    import torch
    rows, cols = _map_tensor(logodds, torch.int16, "logodds")
    _map_tensor(last_seen, torch.int32, "last_seen", like=logodds)
    if pen is not None:
        _map_tensor(pen, torch.uint8, "pen", like=logodds)
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.uint8, device=logodds.device)
    else:
        _map_tensor(out, torch.uint8, "out", like=logodds)
    for v, what in ((occupied, "occupied"), (free, "free")):
        if isinstance(v, bool) or int(v) != v or abs(v) > 2 ** 31 - 1:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    with torch.cuda.device(logodds.device):
        rc = frontier_lib().sv_frontier_cells_device(logodds.data_ptr(), last_seen.data_ptr(), _ptr(pen), rows, cols, int(occupied), int(free), out.data_ptr(),
                                                     torch.cuda.current_stream(logodds.device).cuda_stream)
    _check(rc, "sv_frontier_cells_device")
    return out


class FrontierResult(_Result):
    """What frontier_clusters returns, tensors on the mask's device: label int32 [rows,cols] (-1 on non-members, else the least linear
    index of the cell's 8-connected component), clusters int32 [capacity,8] = (label, size, rep_r, rep_c, r0, c0, r1, c1) per kept
    component in ascending order of label (-1 past the written rows), sums int64 [capacity,2] = (sum_r, sum_c), info int32 [4] = (kept
    components, all components, members, rows written) and workspace (the uint8 tensor the call worked in)."""
    __slots__ = ("label", "clusters", "sums", "info", "workspace")


def frontier_clusters(mask, min_cells=1, capacity=1024, out=None, workspace=None):
    """The connected clusters of a byte mask - the definition of stereo_vision.sv.frontier_clusters on the GPU, bit for bit: mask a
    contiguous CUDA uint8 tensor [rows,cols] (frontier_cells', or the caller's own: a member is a non-zero byte; rows x cols <=
    8 000 000), min_cells in 1 .. 8 000 000, capacity in 1 .. 65535 rows.  out: a FrontierResult (or a tuple (label, clusters, sums,
    info)) of contiguous tensors of the right shapes to write into; workspace: a uint8 tensor of at least
    sv_frontier_clusters_workspace's bytes to reuse.  -> FrontierResult; enqueued on torch's current stream - four memsets and nine
    kernels - and not waited for."""
    import torch
    rows, cols = _map_tensor(mask, torch.uint8, "mask")
    dev = mask.device
    if rows * cols > 8000000:
        raise ValueError("a mask of %d x %d cells: at most 8 000 000, so that a linear index stays below 2^23" % (rows, cols))
    for v, lo, hi, what in ((min_cells, 1, 8000000, "min_cells"), (capacity, 1, 65535, "capacity")):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    capacity = int(capacity)
    shapes = (("label", (rows, cols), torch.int32), ("clusters", (capacity, 8), torch.int32), ("sums", (capacity, 2), torch.int64), ("info", (4,), torch.int32))
    if out is None:
        given = [torch.empty(shape, dtype=dtype, device=dev) for _, shape, dtype in shapes]
    else:
        given = [getattr(out, name) for name, _, _ in shapes] if isinstance(out, FrontierResult) else list(out)
        if len(given) != 4:
            raise ValueError("out must be a FrontierResult or (label, clusters, sums, info)")
        for t, (name, shape, dtype) in zip(given, shapes):
            if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError("out: %s must be a contiguous %s tensor %s on the device of mask" % (name, str(dtype).replace("torch.", ""), list(shape)))
    L = frontier_lib()
    nbytes = ctypes.c_size_t()
    _check(L.sv_frontier_clusters_workspace(rows, cols, capacity, ctypes.byref(nbytes)), "sv_frontier_clusters_workspace")
    if workspace is None:
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    elif not (isinstance(workspace, torch.Tensor) and workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous()
              and workspace.numel() >= nbytes.value):
        raise ValueError("workspace must be a contiguous uint8 tensor of at least %d bytes on the device of mask" % nbytes.value)
    label, clusters, sums, info = given
    with torch.cuda.device(dev):
        rc = L.sv_frontier_clusters_device(mask.data_ptr(), rows, cols, int(min_cells), capacity, label.data_ptr(), clusters.data_ptr(), sums.data_ptr(),
                                           info.data_ptr(), workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_frontier_clusters_device")
    return FrontierResult(label=label, clusters=clusters, sums=sums, info=info, workspace=workspace)


def debug_frontier(variant=0, counters=None):
    """sv_debug_frontier: how frontier_clusters labels (0: tiles in LDS, then their seams; 1: no tile phase, every link through global
    memory) and a CUDA int64 [2] tensor (or None) that receives the atomic minima issued on global memory and the tiles that held a
    member.  Process-wide; a test hook."""
    return int(frontier_lib().sv_debug_frontier(int(variant), None if counters is None else counters.data_ptr()))


def view_lib():
    """The library with the signatures of group (P) declared."""
    return _bind("view")


class ViewResult(_Result):
    """What occupancy_view returns, tensors on the map's device: counts int32 [G,P,3] = (unknown, free, occupied) - the distinct cells
    the rays of a candidate see, by state -, end_cells int16 [G,P,n_rays,2] = (row, col) of each ray's last visible cell, (-1, -1) for
    an invalid one, status uint8 [G,P,n_rays] (stereo_vision.sv.VIEW_FULL .. VIEW_INVALID), best int32 [G] (the lowest p with the
    most unknown cells), best_score int32 [G] (that count, -1 where every candidate is invalid) and workspace (the uint8 tensor the call
    worked in)."""
    __slots__ = ("counts", "end_cells", "status", "best", "best_score", "workspace")


def occupancy_view(logodds, last_seen, map, poses, ends, reach, occupied, free, max_unknown=0, out=None, workspace=None):
    """The expected view of a world map from candidate poses - the definition of stereo_vision.sv.occupancy_view on the GPU, bit for bit,
    in three kernels: logodds a contiguous CUDA int16 tensor [rows,cols] and last_seen an int32 tensor of the same shape on the same
    device, map an SvOccupancyMapSpec or a dict of its nine words, poses float64 [G,P,4] = (tx, ty, c, s) with G * P <= 65535 and ends
    float64 [n_rays,2] (stereo_vision.sv.view_rays', with its reach) - numpy arrays, uploaded once, or tensors on the device -, occupied
    and free the thresholds of the state, max_unknown in 0 .. 255.  out: a ViewResult (or a tuple (counts, end_cells, status, best,
    best_score)) of contiguous tensors of the right shapes to write into; workspace: a uint8 tensor of at least sv_view_workspace's bytes
    to reuse.  -> ViewResult; enqueued on torch's current stream, not waited for; nothing dense is read back."""
    import torch
    from .stereo_vision.sv import VIEW_POSES_MAX, VIEW_RAYS_MAX, VIEW_REACH_MAX, occupancy_map_words
    words = occupancy_map_words(map)
    rows, cols = words["rows"], words["cols"]
    if _map_tensor(logodds, torch.int16, "logodds") != (rows, cols):
        raise ValueError("logodds must be [%d,%d] as the map's words say, got %s" % (rows, cols, tuple(logodds.shape)))
    _map_tensor(last_seen, torch.int32, "last_seen", like=logodds)
    dev = logodds.device
    p, e = _device_poses(poses, dev), _device_poses(ends, dev)
    if p.dim() != 3 or p.shape[2] != 4 or p.shape[1] < 1 or p.shape[0] * p.shape[1] > VIEW_POSES_MAX:
        raise ValueError("poses must be [G,P,4] with P >= 1 and G * P <= 65535, got %s" % (tuple(p.shape),))
    if e.dim() != 2 or e.shape[1] != 2 or not 1 <= e.shape[0] <= VIEW_RAYS_MAX:
        raise ValueError("ends must be [n_rays,2] with 1 <= n_rays <= 1024, got %s" % (tuple(e.shape),))
    for v, lo, hi, what in ((reach, 1, VIEW_REACH_MAX, "reach"), (max_unknown, 0, 255, "max_unknown"), (occupied, -2 ** 31, 2 ** 31 - 1, "occupied"),
                            (free, -2 ** 31, 2 ** 31 - 1, "free")):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    G, P, n_rays = p.shape[0], p.shape[1], e.shape[0]
    shapes = (("counts", (G, P, 3), torch.int32), ("end_cells", (G, P, n_rays, 2), torch.int16), ("status", (G, P, n_rays), torch.uint8),
              ("best", (G,), torch.int32), ("best_score", (G,), torch.int32))
    if out is None:
        given = [torch.empty(shape, dtype=dtype, device=dev) for _, shape, dtype in shapes]
    else:
        given = [getattr(out, name) for name, _, _ in shapes] if isinstance(out, ViewResult) else list(out)
        if len(given) != 5:
            raise ValueError("out must be a ViewResult or (counts, end_cells, status, best, best_score)")
        for t, (name, shape, dtype) in zip(given, shapes):
            if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
                raise ValueError("out: %s must be a contiguous %s tensor %s on the device of logodds" % (name, str(dtype).replace("torch.", ""), list(shape)))
    L = view_lib()
    nbytes = ctypes.c_size_t()
    _check(L.sv_view_workspace(rows, cols, ctypes.byref(nbytes)), "sv_view_workspace")
    if workspace is None:
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    elif not (isinstance(workspace, torch.Tensor) and workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous()
              and workspace.numel() >= nbytes.value):
        raise ValueError("workspace must be a contiguous uint8 tensor of at least %d bytes on the device of logodds" % nbytes.value)
    counts, end_cells, status, best, best_score = given
    spec = _occupancy_map_struct(words)
    with torch.cuda.device(dev):
        rc = L.sv_view_device(logodds.data_ptr(), last_seen.data_ptr(), ctypes.byref(spec), _ptr(p), G, P, e.data_ptr(), n_rays, int(reach), int(occupied), int(free),
                              int(max_unknown), _ptr(counts), _ptr(end_cells), _ptr(status), _ptr(best), _ptr(best_score), workspace.data_ptr(), workspace.numel(),
                              torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_view_device")
    return ViewResult(counts=counts, end_cells=end_cells, status=status, best=best, best_score=best_score, workspace=workspace)


def debug_view(variant=0, stages=3):
    """sv_debug_view: the LDS window of occupancy_view's workgroups (0: sized by the call's reach; 1: always 509 cells a side) and the
    kernels a call enqueues (3: all; 1: the state plane alone; 2: without the best).  Process-wide; a test and measurement hook."""
    return int(view_lib().sv_debug_view(int(variant), int(stages)))


def voxel_map_lib():
    """The library with the signatures of group (Q) declared."""
    return _bind("voxel_map")


VOXEL_MAP_ROW_FIELDS = ("xyz", "color", "cell", "n", "m", "first_seq", "last_seq", "key")  # of voxel_map_rows' dict, besides count


def voxel_map_spec(params):
    """-> SvVoxelMapSpec from a dict with lo, hi, size and capacity (stereo_vision.sv.voxel_map_params', whose checks are made again:
    ValueError for a bad word)."""
    from .stereo_vision.sv import voxel_map_params
    w = voxel_map_params(params["lo"], params["hi"], params["size"], params["capacity"])
    spec = SvVoxelMapSpec()
    spec.lo[:] = w["lo"]
    spec.hi[:] = w["hi"]
    spec.size, spec.capacity = w["size"], w["capacity"]
    return spec


def voxel_map_slot_of(key, slots):
    """sv_voxel_map_slot_of for one key: the slot at which the table's probing starts.  Needs no device."""
    h = int(voxel_map_lib().sv_voxel_map_slot_of(int(key), int(slots)))
    if h < 0:
        raise ValueError("slots must be a power of two in 2 .. 2^32, got %r" % (slots,))
    return h


def _voxel_map_buffer(buf, spec):
    """The map's buffer, checked: a contiguous CUDA int64 tensor of at least sv_voxel_map_bytes(capacity) bytes -> its bytes."""
    import torch
    need = voxel_map_lib().sv_voxel_map_bytes(spec.capacity)
    if not (isinstance(buf, torch.Tensor) and buf.is_cuda and buf.dtype == torch.int64 and buf.is_contiguous() and buf.numel() * 8 >= need):
        raise ValueError("the map must be a contiguous CUDA int64 tensor of at least %d bytes (voxel_map_new)" % need)
    return buf.numel() * 8


def voxel_map_new(params, device="cuda"):
    """-> the buffer of an empty voxel map for `params` on `device`: an int64 tensor of sv_voxel_map_bytes(capacity) bytes - a head of 32
    bytes, sv_voxel_map_slots(capacity) entries of 88 bytes, the read-out's scratch -, cleared on torch's current stream."""
    import torch
    spec = voxel_map_spec(params)
    nbytes = voxel_map_lib().sv_voxel_map_bytes(spec.capacity)
    buf = torch.empty((nbytes // 8,), dtype=torch.int64, device=device)  # torch's allocations start on 512 bytes
    return voxel_map_clear(buf, params)


def voxel_map_clear(buf, params):
    """Empties the map in `buf` (sv_voxel_map_clear_device) on torch's current stream; -> buf."""
    import torch
    spec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, spec)
    with torch.cuda.device(buf.device):
        rc = voxel_map_lib().sv_voxel_map_clear_device(buf.data_ptr(), nbytes, ctypes.byref(spec), torch.cuda.current_stream(buf.device).cuda_stream)
    _check(rc, "sv_voxel_map_clear_device")
    return buf


def voxel_map_poses(poses, dev):
    """The poses of voxel_map_insert as a contiguous float64 [B,12] tensor on dev: [B,12] (R row-major, then t) as they are, the occupancy
    map's [B,4] = (tx, ty, c, s) expanded as stereo_vision.sv.voxel_map_pose does with z = 0; numpy arrays are uploaded once."""
    import torch
    if not isinstance(poses, torch.Tensor):
        from .stereo_vision.sv import voxel_map_pose_words
        return torch.from_numpy(voxel_map_pose_words(poses)).to(dev)
    if poses.device != dev or poses.dtype != torch.float64 or poses.dim() != 2 or poses.shape[1] not in (4, 12):
        raise ValueError("poses must be float64 [B,12] or [B,4] on the device (%s) of the map" % (dev,))
    if poses.shape[1] == 12:
        return poses.contiguous()
    tx, ty, c, s = poses.unbind(1)
    zero, one = torch.zeros_like(tx), torch.ones_like(tx)
    return torch.stack([c, -s, zero, s, c, zero, zero, zero, one, tx, ty, zero], 1).contiguous()


def voxel_map_insert(buf, params, xyz, color, n, counts, poses, seq0=0):
    """Adds B frames of rows to the voxel map in `buf` - the definition of stereo_vision.sv.voxel_map_insert on the GPU, one kernel: xyz
    CUDA float32 or float64 [B,cap,3], color uint8 [B,cap,4] or None, n int32 [B,cap] or None, counts int32 [B] - what
    voxel_cloud_from_disparity and compact_cloud_from_disparity return, on the map's device -, poses float64 [B,12] or [B,4] (numpy, or a
    tensor on the device), seq0 the sequence number of frame 0.  counts and poses are read on the device.  Enqueued on torch's current
    stream, not waited for; -> buf."""
    import torch
    spec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, spec)
    dev = buf.device
    if not (isinstance(xyz, torch.Tensor) and xyz.device == dev and xyz.dtype in (torch.float32, torch.float64) and xyz.dim() == 3 and xyz.shape[2] == 3):
        raise ValueError("xyz must be a float32 or float64 tensor [B,cap,3] on the map's device")
    B, cap = int(xyz.shape[0]), int(xyz.shape[1])
    for t, name, dtype, shape in ((color, "color", torch.uint8, (B, cap, 4)), (n, "n", torch.int32, (B, cap)), (counts, "counts", torch.int32, (B,))):
        if t is None and name != "counts":
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape):
            raise ValueError("%s must be a %s tensor %s on the map's device" % (name, str(dtype).replace("torch.", ""), list(shape)))
    if B > 65535:
        raise ValueError("at most 65535 frames per call, got %d" % B)
    if isinstance(seq0, bool) or int(seq0) != seq0 or seq0 < 0 or seq0 + B > 2 ** 31 - 1:
        raise ValueError("the sequence numbers seq0 .. seq0 + B - 1 must stay in 0 .. 2^31 - 2, got seq0 = %r" % (seq0,))
    p = voxel_map_poses(poses, dev)
    if p.shape[0] != B:
        raise ValueError("poses must hold one pose per frame: %d, got %d" % (B, p.shape[0]))
    xyz, counts = xyz.contiguous(), counts.contiguous()
    color = None if color is None else color.contiguous()
    if color is not None and color.data_ptr() % 4:  # the C entry moves a colour as one dword
        color = color.clone()
    n = None if n is None else n.contiguous()
    with torch.cuda.device(dev):
        rc = voxel_map_lib().sv_voxel_map_insert_device(buf.data_ptr(), nbytes, ctypes.byref(spec), _ptr(xyz), 0 if xyz.dtype == torch.float32 else 1, _ptr(color),
                                                        _ptr(n), _ptr(counts), _ptr(p), B, cap, int(seq0), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_map_insert_device")
    return buf


def voxel_map_rows(buf, params, min_n=1, min_rows=1, since=0, dtype="f32", capacity=None, sort=True):
    """The voxels of the map in `buf` with n >= min_n, m >= min_rows and last_seq >= since (sv_voxel_map_rows_device: three kernels) as a
    dict of tensors on the map's device - xyz float32 or float64 ("f64") [V,3], color uint8 [V,4], cell int32 [V,3], n int64 [V], m
    int64 [V], first_seq int32 [V], last_seq int32 [V], key int64 [V] - and count.  capacity: the rows of the output tensors (None: the
    map's capacity, which always suffices).
    sort=True: count is read back (the one synchronisation), the rows are cut at it and ordered by key with torch.sort and a gather: the
    result equals stereo_vision.sv.voxel_map_rows' in shape, dtype and bits; count is an int, -1 (and no rows) for an overflowed map;
    StereoError where count exceeds `capacity`.
    sort=False: what the C entry wrote, not waited for: tensors of `capacity` rows in slot order - which depends on the schedule of the
    inserts - of which the first count are rows (all of them only while count <= capacity), and count an int32 tensor [1]."""
    import torch
    from .stereo_vision.sv import CLOUD_DTYPES
    spec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, spec)
    if dtype not in CLOUD_DTYPES:
        raise ValueError("dtype must be one of %s, got %r" % (sorted(CLOUD_DTYPES), dtype))
    for v, what in ((min_n, "min_n"), (min_rows, "min_rows")):
        if isinstance(v, bool) or int(v) != v or not -2 ** 63 <= v < 2 ** 63:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    cap = spec.capacity if capacity is None else capacity
    if isinstance(cap, bool) or int(cap) != cap or not 0 <= cap < 2 ** 31:
        raise ValueError("capacity must be an integer in 0 .. 2^31 - 1, got %r" % (capacity,))
    cap, dev = int(cap), buf.device
    shapes = {"xyz": ((cap, 3), torch.float32 if dtype == "f32" else torch.float64), "color": ((cap, 4), torch.uint8), "cell": ((cap, 3), torch.int32),
              "n": ((cap,), torch.int64), "m": ((cap,), torch.int64), "first_seq": ((cap,), torch.int32), "last_seq": ((cap,), torch.int32),
              "key": ((cap,), torch.int64)}
    out = {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = voxel_map_lib().sv_voxel_map_rows_device(buf.data_ptr(), nbytes, ctypes.byref(spec), int(min_n), int(min_rows), int(since), CLOUD_DTYPES[dtype], cap,
                                                      *[_ptr(out[k]) for k in VOXEL_MAP_ROW_FIELDS], count.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_map_rows_device")
    if not sort:
        out["count"] = count
        return out
    V = int(count.item())
    if V > cap:
        raise StereoError("%d voxels qualify but the output holds %d rows: raise the capacity" % (V, cap))
    order = torch.sort(out["key"][:max(V, 0)]).indices
    out = {k: t[:max(V, 0)][order] for k, t in out.items()}
    out["count"] = V
    return out


def voxel_map_stats(buf):
    """(claimed voxels, dropped rows, overflowed) of the map in `buf`: its head, read back - this synchronises."""
    head = buf[:2].cpu().numpy()
    words = head.view(np.uint32)
    return int(words[0]), int(head.view(np.uint64)[1]), bool(words[1])


def debug_voxel_map(combine=True, counters=None):
    """sv_debug_voxel_map: the wavefront merge of the insert kernel on / off and a CUDA int64 [2] tensor (or None) that receives the table
    updates and the atomic instructions they issued.  Process-wide; a test and measurement hook."""
    return int(voxel_map_lib().sv_debug_voxel_map(1 if combine else 0, None if counters is None else counters.data_ptr()))


def voxel_match_lib():
    """The library with the signatures of group (R) declared."""
    return _bind("voxel_match")


class VoxelMatchResult(_Result):
    """What voxel_map_match returns, tensors on the map's device: inside, hits int32 [B,P], weight, d2 int64 [B,P] (all four None where
    not asked for), best int32 [B], best_weight and best_d2 int64 [B]."""
    __slots__ = ("inside", "hits", "weight", "d2", "best", "best_weight", "best_d2")


def voxel_match_poses(poses, B, dev):
    """The candidates of voxel_map_match as a contiguous float64 [B,P,12] tensor on dev: a numpy array - uploaded once - or a tensor on
    dev; [P,12] accepted for one frame."""
    import torch
    p = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).to(dev)
    if p.device != dev or p.dtype != torch.float64:
        raise ValueError("poses must be float64 on the device (%s) of the map" % (dev,))
    if p.dim() == 2 and B == 1:
        p = p.unsqueeze(0)
    if p.dim() != 3 or p.shape[0] != B or p.shape[2] != 12:
        raise ValueError("poses must be [%d,P,12], got %s" % (B, tuple(p.shape)))
    return p.contiguous()


def voxel_map_match(buf, params, xyz, n, counts, poses, min_n=1, min_rows=1, since=0, want_sums=True):
    """The rows of B frames - xyz CUDA float32 or float64 [B,cap,3], n int32 [B,cap] or None, counts int32 [B], as voxel_map_insert takes
    them - scored against the voxel map in `buf` at P candidate poses per frame (float64 [B,P,12], stereo_vision.sv.voxel_map_pose of
    voxel_map_pose_window's rows or any rigid poses; numpy or a tensor on the map's device; [P,12] accepted for one frame) - the
    definition of stereo_vision.sv.voxel_map_match on the GPU, bit for bit (sv_voxel_match_device: three kernels): per candidate the rows
    that fall into the map's box, those that fall into a voxel with n >= min_n, m >= min_rows and last_seq >= since, their weight and
    their squared sub-cell distance to the voxels' means, and per frame the candidate with the largest weight (then the smallest d2, then
    the lowest index).  want_sums=False leaves the four per-candidate tensors out.  The map is not changed, nothing is read back, and the
    workspace comes from torch's allocator, which keeps it for the next call of the shape.  -> VoxelMatchResult; enqueued on torch's
    current stream, not waited for."""
    import torch
    spec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, spec)
    dev = buf.device
    if not (isinstance(xyz, torch.Tensor) and xyz.device == dev and xyz.dtype in (torch.float32, torch.float64) and xyz.dim() == 3 and xyz.shape[2] == 3):
        raise ValueError("xyz must be a float32 or float64 tensor [B,cap,3] on the map's device")
    B, cap = int(xyz.shape[0]), int(xyz.shape[1])
    for t, name, dtype, shape in ((n, "n", torch.int32, (B, cap)), (counts, "counts", torch.int32, (B,))):
        if t is None and name != "counts":
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape):
            raise ValueError("%s must be a %s tensor %s on the map's device" % (name, str(dtype).replace("torch.", ""), list(shape)))
    p = voxel_match_poses(poses, B, dev)
    n_poses = int(p.shape[1])
    if B > 65535 or not 1 <= n_poses <= 65535 or B * n_poses >= 2 ** 31:
        raise ValueError("at most 65535 frames of 1 .. 65535 poses each and fewer than 2^31 in all, got %d x %d" % (B, n_poses))
    for v, what in ((min_n, "min_n"), (min_rows, "min_rows")):
        if isinstance(v, bool) or int(v) != v or not -2 ** 63 <= v < 2 ** 63:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    res = VoxelMatchResult(best=torch.empty((B,), dtype=torch.int32, device=dev), best_weight=torch.empty((B,), dtype=torch.int64, device=dev),
                           best_d2=torch.empty((B,), dtype=torch.int64, device=dev))
    if want_sums:
        res.inside, res.hits = (torch.empty((B, n_poses), dtype=torch.int32, device=dev) for _ in range(2))
        res.weight, res.d2 = (torch.empty((B, n_poses), dtype=torch.int64, device=dev) for _ in range(2))
    if B == 0:  # nothing to enqueue
        return res
    L = voxel_match_lib()
    need = ctypes.c_size_t()
    _check(L.sv_voxel_match_workspace(cap, n_poses, B, ctypes.byref(need)), "sv_voxel_match_workspace")
    ws = torch.empty((need.value + 15) // 16 * 2, dtype=torch.int64, device=dev)
    xyz, counts = xyz.contiguous(), counts.contiguous()
    n = None if n is None else n.contiguous()
    out = [res.inside, res.hits, res.weight, res.d2] if want_sums else [None] * 4
    with torch.cuda.device(dev):
        rc = L.sv_voxel_match_device(buf.data_ptr(), nbytes, ctypes.byref(spec), _ptr(xyz), 0 if xyz.dtype == torch.float32 else 1, _ptr(n), counts.data_ptr(),
                                     p.data_ptr(), B, cap, n_poses, int(min_n), int(min_rows), int(since), *[None if t is None else t.data_ptr() for t in out],
                                     res.best.data_ptr(), res.best_weight.data_ptr(), res.best_d2.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                     torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_match_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def debug_voxel_match(group=0):
    """sv_debug_voxel_match: the candidates a workgroup of the score kernel walks (0: the call chooses; a power of two in 1 .. 64).
    Process-wide; a test hook."""
    return int(voxel_match_lib().sv_debug_voxel_match(int(group)))


def voxel_carry_lib():
    """The library with the signatures of group (S) declared."""
    return _bind("voxel_carry")


def voxel_map_carry(dst_buf, dst_params, src_buf, src_params, shift=(0, 0, 0), min_n=1, min_rows=1, since=0):
    """Adds the voxels of the map in src_buf - those with n >= min_n, m >= min_rows and last_seq >= since, their cells moved by `shift`
    whole cells (three integers in -2^20 .. 2^20) - into the map in dst_buf: the definition of stereo_vision.sv.voxel_map_carry on the
    GPU, bit for bit (sv_voxel_map_carry_device: two kernels).  Both maps are voxel_map_new's buffers with their params, on one device,
    of bit-equal size and sharing no memory; src is only read.  -> an int64 [4] tensor on the device: carried (-1 where either map was
    overflowed: nothing is carried), filtered, outside, claimed - stereo_vision.sv.VOXEL_CARRY_STATS.  Enqueued on torch's current
    stream, not waited for; no other work on either map may run on another stream meanwhile."""
    import torch
    from .stereo_vision.sv import VOXEL_CARRY_SHIFT_MAX
    dst_spec, src_spec = voxel_map_spec(dst_params), voxel_map_spec(src_params)
    dst_bytes, src_bytes = _voxel_map_buffer(dst_buf, dst_spec), _voxel_map_buffer(src_buf, src_spec)
    if src_buf.device != dst_buf.device:
        raise ValueError("the two maps must lie on one device, got %s and %s" % (dst_buf.device, src_buf.device))
    try:
        shift = [int(v) if not isinstance(v, bool) and int(v) == v else None for v in shift]
    except (TypeError, ValueError):
        shift = [None]
    if len(shift) != 3 or any(v is None or abs(v) > VOXEL_CARRY_SHIFT_MAX for v in shift):
        raise ValueError("shift must be three integers in -2^20 .. 2^20")
    for v, what in ((min_n, "min_n"), (min_rows, "min_rows")):
        if isinstance(v, bool) or int(v) != v or not -2 ** 63 <= v < 2 ** 63:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    dev = dst_buf.device
    stats = torch.empty((4,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = voxel_carry_lib().sv_voxel_map_carry_device(dst_buf.data_ptr(), dst_bytes, ctypes.byref(dst_spec), src_buf.data_ptr(), src_bytes, ctypes.byref(src_spec),
                                                         shift[0], shift[1], shift[2], int(min_n), int(min_rows), int(since), stats.data_ptr(),
                                                         torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_map_carry_device")
    return stats


def voxel_repose_lib():
    """The library with the signatures of group (AD) declared."""
    return _bind("voxel_repose")


def voxel_map_repose(dst_buf, dst_params, src_buf, src_params, corr, seq0=0, min_n=1, min_rows=1, since=0):
    """Adds the voxels of the map in src_buf - those with n >= max(min_n, 1), m >= min_rows and last_seq >= since, each moved by the rigid
    correction corr[min(max(last_seq - seq0, 0), K - 1)] - into the map in dst_buf: the definition of stereo_vision.sv.voxel_map_repose on
    the GPU, bit for bit (sv_voxel_repose_device: two kernels).  Both maps are voxel_map_new's buffers with their params, on one device
    and sharing no memory; box, size and capacity may differ; src is only read.  corr: float64 [K,12], K in 1 .. 2^22 - a numpy array,
    uploaded here, or a tensor on the maps' device.  -> an int64 [4] tensor on the device: carried (-1 where either map was overflowed:
    nothing is carried), filtered, outside, claimed - stereo_vision.sv.VOXEL_CARRY_STATS.  Enqueued on torch's current stream, not waited
    for; no other work on either map may run on another stream meanwhile."""
    import torch
    from .stereo_vision.sv import VOXEL_MAP_SEQ_MAX, VOXEL_REPOSE_CORR_MAX
    dst_spec, src_spec = voxel_map_spec(dst_params), voxel_map_spec(src_params)
    dst_bytes, src_bytes = _voxel_map_buffer(dst_buf, dst_spec), _voxel_map_buffer(src_buf, src_spec)
    if src_buf.device != dst_buf.device:
        raise ValueError("the two maps must lie on one device, got %s and %s" % (dst_buf.device, src_buf.device))
    dev = dst_buf.device
    if not isinstance(corr, torch.Tensor):
        try:
            corr = torch.from_numpy(np.ascontiguousarray(corr, dtype=np.float64)).to(dev)
        except (TypeError, ValueError):
            raise ValueError("corr must be float64 [K,12]")
    if corr.device != dev or corr.dtype != torch.float64 or corr.dim() != 2 or corr.shape[1] != 12 or not 1 <= corr.shape[0] <= VOXEL_REPOSE_CORR_MAX:
        raise ValueError("corr must be float64 [K,12] with K in 1 .. 2^22 on the device (%s) of the maps" % (dev,))
    corr = corr.contiguous()
    if isinstance(seq0, bool) or int(seq0) != seq0 or not 0 <= seq0 <= VOXEL_MAP_SEQ_MAX:
        raise ValueError("seq0 must be an integer in 0 .. 2^31 - 2, got %r" % (seq0,))
    for v, what in ((min_n, "min_n"), (min_rows, "min_rows")):
        if isinstance(v, bool) or int(v) != v or not -2 ** 63 <= v < 2 ** 63:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    stats = torch.empty((4,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = voxel_repose_lib().sv_voxel_repose_device(dst_buf.data_ptr(), dst_bytes, ctypes.byref(dst_spec), src_buf.data_ptr(), src_bytes, ctypes.byref(src_spec),
                                                       corr.data_ptr(), int(corr.shape[0]), int(seq0), int(min_n), int(min_rows), int(since), stats.data_ptr(),
                                                       torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_repose_device")
    return stats  # corr goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def voxel_carve_lib():
    """The library with the signatures of group (T) declared."""
    return _bind("voxel_carve")


class VoxelCarveResult(_Result):
    """What voxel_map_carve returns, tensors on the map's device: stats int64 [4] - rays (-1 for an overflowed map: nothing was done),
    steps, touched, carved (stereo_vision.sv.VOXEL_CARVE_STATS) - and miss int64 [slots], the weight counted against the voxel of every
    slot of the table.  Neither is waited for."""
    __slots__ = ("stats", "miss")


def voxel_carve_miss(buf, params):
    """-> the per-slot tensor voxel_map_carve writes: int64 [sv_voxel_map_slots(capacity)] on the device of the map in `buf`."""
    import torch
    slots = int(voxel_map_lib().sv_voxel_map_slots(voxel_map_spec(params).capacity))
    return torch.empty((slots,), dtype=torch.int64, device=buf.device)


def voxel_map_carve(buf, params, xyz, n, counts, poses, origin=(0.0, 0.0, 0.0), seq0=0, reach=1023, margin=1, min_miss=1, ratio=0, apply=True, miss=None):
    """Carves free space out of the voxel map in `buf` along the sight lines of B frames - the definition of
    stereo_vision.sv.voxel_map_carve on the GPU, bit for bit (sv_voxel_carve_device: three kernels): xyz, n, counts, poses and seq0 as
    voxel_map_insert takes them (usually the insert's own arguments, behind it), origin the sensor's centre in the frame's axes (three
    finite numbers, read here), reach 1 .. 1023 and margin 0 .. 255 in cells, min_miss >= 1, ratio 0 .. 65535 in 1 / 256 of a voxel's
    weight.  A voxel no later frame has seen, with enough weight of rays through it, is emptied under `apply`: its key stays in the table
    - a tombstone that every call skips at min_n >= 1 and the next carry drops; until then the read-out is defined for min_n >= 1 only.
    miss: voxel_carve_miss' tensor to write into (None: a new one).  -> VoxelCarveResult; enqueued on torch's current stream, not waited
    for, and no other work on the map may run on another stream meanwhile."""
    import torch
    from .stereo_vision.sv import VOXEL_CARVE_MARGIN_MAX, VOXEL_CARVE_REACH_MAX
    spec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, spec)
    dev = buf.device
    if not (isinstance(xyz, torch.Tensor) and xyz.device == dev and xyz.dtype in (torch.float32, torch.float64) and xyz.dim() == 3 and xyz.shape[2] == 3):
        raise ValueError("xyz must be a float32 or float64 tensor [B,cap,3] on the map's device")
    B, cap = int(xyz.shape[0]), int(xyz.shape[1])
    for t, name, dtype, shape in ((n, "n", torch.int32, (B, cap)), (counts, "counts", torch.int32, (B,))):
        if t is None and name != "counts":
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape):
            raise ValueError("%s must be a %s tensor %s on the map's device" % (name, str(dtype).replace("torch.", ""), list(shape)))
    if B > 65535:
        raise ValueError("at most 65535 frames per call, got %d" % B)
    if isinstance(seq0, bool) or int(seq0) != seq0 or seq0 < 0 or seq0 + B > 2 ** 31 - 1:
        raise ValueError("the sequence numbers seq0 .. seq0 + B - 1 must stay in 0 .. 2^31 - 2, got seq0 = %r" % (seq0,))
    for v, what, lo, hi in ((reach, "reach", 1, VOXEL_CARVE_REACH_MAX), (margin, "margin", 0, VOXEL_CARVE_MARGIN_MAX), (min_miss, "min_miss", 1, 2 ** 63 - 1),
                            (ratio, "ratio", 0, 65535), (apply, "apply", 0, 1)):
        if (isinstance(v, bool) and what != "apply") or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    try:
        o = np.array([float(v) for v in origin], np.float64)
    except (TypeError, ValueError):
        o = np.zeros(0)
    if o.shape != (3,) or not np.isfinite(o).all():
        raise ValueError("origin must be three finite numbers, got %r" % (origin,))
    p = voxel_map_poses(poses, dev)
    if p.shape[0] != B:
        raise ValueError("poses must hold one pose per frame: %d, got %d" % (B, p.shape[0]))
    slots = int(voxel_map_lib().sv_voxel_map_slots(spec.capacity))
    if miss is None:
        miss = torch.empty((slots,), dtype=torch.int64, device=dev)
    elif not (isinstance(miss, torch.Tensor) and miss.device == dev and miss.dtype == torch.int64 and miss.is_contiguous() and tuple(miss.shape) == (slots,)):
        raise ValueError("miss must be a contiguous int64 tensor [%d] on the map's device (voxel_carve_miss)" % slots)
    res = VoxelCarveResult(stats=torch.empty((4,), dtype=torch.int64, device=dev), miss=miss)
    xyz, counts = xyz.contiguous(), counts.contiguous()
    n = None if n is None else n.contiguous()
    with torch.cuda.device(dev):
        rc = voxel_carve_lib().sv_voxel_carve_device(buf.data_ptr(), nbytes, ctypes.byref(spec), _ptr(xyz), 0 if xyz.dtype == torch.float32 else 1, _ptr(n),
                                                     _ptr(counts), _ptr(p), o.ctypes.data, B, cap, int(seq0), int(reach), int(margin), int(min_miss), int(ratio),
                                                     int(apply), miss.data_ptr(), res.stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_carve_device")
    return res


def voxel_carve_touched(buf, params, miss):
    """-> (key, miss) of the slots with miss > 0, ordered by key: two int64 tensors on the map's device, what
    stereo_vision.sv.voxel_map_carve returns as "key" and "miss".  The keys are read through a strided int64 view of the map's buffer -
    the first word of each entry of eleven behind the head of four.  Reads the number of touched slots back: this synchronises."""
    import torch
    spec = voxel_map_spec(params)
    _voxel_map_buffer(buf, spec)
    slots = int(voxel_map_lib().sv_voxel_map_slots(spec.capacity))
    if not (isinstance(miss, torch.Tensor) and miss.device == buf.device and miss.dtype == torch.int64 and tuple(miss.shape) == (slots,)):
        raise ValueError("miss must be the int64 tensor [%d] of voxel_map_carve on the map's device" % slots)
    keys = buf[4:].as_strided((slots,), (11,))
    at = torch.nonzero(miss > 0).reshape(-1)
    order = torch.sort(keys[at]).indices
    return keys[at][order], miss[at][order]


def voxel_render_lib():
    """The library with the signatures of group (U) declared."""
    return _bind("voxel_render")


class VoxelRenderResult(_Result):
    """What voxel_map_render returns, tensors on the map's device: depth int32 [V,H,W] (zq, -1 where no voxel covers the pixel), key int64
    [V,H,W] (the winner's, or -1), color uint8 [V,H,W,4] (0), disparity float32 [V,H,W] (-1), stats int64 [V,2] = drawn, covered (-1, 0 for
    an overflowed map), and with `measured` label uint8 [V,H,W] (stereo_vision.sv.VOXEL_RENDER_LABELS) and counts int64 [V,6] - None
    without.  color and disparity are None where they were left out.  None is waited for."""
    __slots__ = ("depth", "key", "color", "disparity", "stats", "label", "counts")


def voxel_render_spec(camera, r_max=4, near=None, far=None):
    """-> SvVoxelRenderSpec from a camera dict (stereo_vision.sv.voxel_render_camera's) and the call's r_max, near and far, after
    stereo_vision.sv.voxel_render_words' checks (ValueError for a bad word)."""
    from .stereo_vision.sv import voxel_render_words
    w = voxel_render_words(camera, r_max, near, far)
    spec = SvVoxelRenderSpec()
    for k in ("f", "cx", "cy", "q32", "q33", "half_px", "near", "far", "width", "height", "r_max"):
        setattr(spec, k, w[k])
    return spec


def voxel_map_render(buf, params, cams, camera, measured=None, tol=1.0, near=None, far=None, r_max=4, min_n=1, min_rows=1, since=0, color=True,
                     disparity=True, out=None):
    """The voxel map in `buf` rendered into V views of one camera - the definition of stereo_vision.sv.voxel_map_render on the GPU, bit
    for bit (sv_voxel_render_device: four kernels): cams float64 [V,12], world to camera (stereo_vision.sv.voxel_render_cams; numpy,
    uploaded once, or a tensor on the map's device), camera a dict of f, cx, cy, q32, q33, half_px, width and height
    (stereo_vision.sv.voxel_render_camera), near < far in cells (None: 1 and 2^20), r_max 0 .. 8 pixels, min_n >= 1, min_rows and since
    the read-out's filters.  measured: a float32 tensor [V,H,W] on the map's device (the engine's D1) to compare the expected disparity
    with, at `tol` pixels: label and counts are then returned too.  color / disparity = False leaves that output out.  out: a
    VoxelRenderResult of an earlier call of the same shapes to write into.  The map is only read.  -> VoxelRenderResult; enqueued on
    torch's current stream, not waited for."""
    import torch
    spec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, spec)
    dev = buf.device
    cam = voxel_render_spec(camera, r_max, near, far)
    H, W = int(cam.height), int(cam.width)
    p = cams if isinstance(cams, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cams, dtype=np.float64)).to(dev)
    if p.device != dev or p.dtype != torch.float64 or p.dim() != 2 or p.shape[1] != 12:
        raise ValueError("cams must be float64 [V,12] on the device (%s) of the map" % (dev,))
    p = p.contiguous()
    V = int(p.shape[0])
    if V > 4096 or V * H * W >= 2 ** 31:
        raise ValueError("at most 4096 views and fewer than 2^31 pixels in all, got %d x %d x %d" % (V, H, W))
    for v, what, lo in ((min_n, "min_n", 1), (min_rows, "min_rows", -2 ** 63)):
        if isinstance(v, bool) or int(v) != v or not lo <= v < 2 ** 63:
            raise ValueError("%s must be an integer >= %d, got %r" % (what, lo, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    if measured is not None:
        if not (isinstance(measured, torch.Tensor) and measured.device == dev and measured.dtype == torch.float32 and tuple(measured.shape) == (V, H, W)):
            raise ValueError("measured must be a float32 tensor [%d,%d,%d] on the map's device" % (V, H, W))
        measured = measured.contiguous()
        if not (isinstance(tol, (int, float)) and tol >= 0):
            raise ValueError("tol must be a number >= 0, got %r" % (tol,))
    shapes = {"depth": ((V, H, W), torch.int32), "key": ((V, H, W), torch.int64), "color": ((V, H, W, 4), torch.uint8), "disparity": ((V, H, W), torch.float32),
              "stats": ((V, 2), torch.int64), "label": ((V, H, W), torch.uint8), "counts": ((V, 6), torch.int64)}
    wanted = [k for k in VoxelRenderResult.__slots__ if not ((k == "color" and not color) or (k == "disparity" and not disparity)
                                                             or (k in ("label", "counts") and measured is None))]
    if out is not None and not isinstance(out, VoxelRenderResult):
        raise ValueError("out must be a VoxelRenderResult")
    res = VoxelRenderResult()
    for k in wanted:
        shape, dtype = shapes[k]
        t = None if out is None else getattr(out, k)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError("out: %s must be a contiguous %s tensor %s on the map's device" % (k, str(dtype).replace("torch.", ""), list(shape)))
        setattr(res, k, t)
    if V == 0:  # nothing to enqueue
        return res
    tol_word = ctypes.c_double(float(tol))
    with torch.cuda.device(dev):
        rc = voxel_render_lib().sv_voxel_render_device(buf.data_ptr(), nbytes, ctypes.byref(spec), ctypes.byref(cam), p.data_ptr(), V, int(min_n), int(min_rows), int(since),
                                                       res.depth.data_ptr(), res.key.data_ptr(), _ptr(res.color), _ptr(res.disparity), _ptr(measured),
                                                       ctypes.addressof(tol_word) if measured is not None else None, _ptr(res.label), res.stats.data_ptr(),
                                                       _ptr(res.counts), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_render_device")
    return res


def debug_voxel_render(groups=0, stages=0):
    """sv_debug_voxel_render: the workgroups of voxel_map_render's two table walks at most (0: the call chooses; 1 .. 2048) and the
    kernels a call enqueues (0: all four; 1 .. 3: the first that many - clear, depth, key).  Returns the groups before.  Process-wide; a
    test and measurement hook."""
    return int(voxel_render_lib().sv_debug_voxel_render(int(groups), int(stages)))


def voxel_flatten_lib():
    """The library with the signatures of group (V) declared."""
    return _bind("voxel_flatten")


class VoxelFlattenResult(_Result):
    """What voxel_map_flatten returns, tensors on the voxel map's device: logodds int16 and last_seen int32 [rows,cols] - the flat map's
    layout, what occupancy_clearance, frontier_cells and occupancy_view take -, floor and top int32 [rows,cols] (zq units, -1 where there
    is none), cells int32 [rows,cols,3] = ground, obstacle and overhead voxels, and stats int64 [8]
    (stereo_vision.sv.VOXEL_FLATTEN_STATS; drawn = -1 for an overflowed map), which stays on the device until it is asked for.  None is
    waited for."""
    __slots__ = ("logodds", "last_seen", "floor", "top", "cells", "stats")


def voxel_flatten_spec(spec):
    """-> SvVoxelFlattenSpec from a dict of its words (stereo_vision.sv.voxel_flatten_params'), after stereo_vision.sv.voxel_flatten_words'
    checks (ValueError for a bad word)."""
    from .stereo_vision.sv import voxel_flatten_words
    out = SvVoxelFlattenSpec()
    for k, v in voxel_flatten_words(spec).items():
        setattr(out, k, v)
    return out


def voxel_map_flatten(buf, params, flat_map, spec, min_n=1, min_rows=1, since=0, out=None):
    """The voxel map in `buf` flattened into the layout of the flat map `flat_map` - the definition of
    stereo_vision.sv.voxel_map_flatten on the GPU, bit for bit (sv_voxel_flatten_device: four or five kernels): flat_map an
    SvOccupancyMapSpec or a dict of its nine words (stereo_vision.sv.occupancy_map_params), at most 8 000 000 cells; spec a dict of the
    height rule's words (stereo_vision.sv.voxel_flatten_params); min_n >= 1, min_rows and since the read-out's filters.  out: a
    VoxelFlattenResult to write into - an earlier call's, or one whose logodds and last_seen are a map's own tensors; a slot that is None
    is allocated.  The voxel map is only read.  -> VoxelFlattenResult; enqueued on torch's current stream, not waited for."""
    import torch
    from .stereo_vision.sv import VOXEL_FLATTEN_CELLS_MAX, occupancy_map_words
    vspec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, vspec)
    dev = buf.device
    words = occupancy_map_words(flat_map)
    rows, cols = words["rows"], words["cols"]
    if rows * cols > VOXEL_FLATTEN_CELLS_MAX:
        raise ValueError("a flat map of %d x %d cells: at most 8 000 000" % (rows, cols))
    fspec = voxel_flatten_spec(spec)
    for v, what, lo in ((min_n, "min_n", 1), (min_rows, "min_rows", -2 ** 63)):
        if isinstance(v, bool) or int(v) != v or not lo <= v < 2 ** 63:
            raise ValueError("%s must be an integer >= %d, got %r" % (what, lo, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    shapes = {"logodds": ((rows, cols), torch.int16), "last_seen": ((rows, cols), torch.int32), "floor": ((rows, cols), torch.int32), "top": ((rows, cols), torch.int32),
              "cells": ((rows, cols, 3), torch.int32), "stats": ((8,), torch.int64)}
    if out is not None and not isinstance(out, VoxelFlattenResult):
        raise ValueError("out must be a VoxelFlattenResult")
    res = VoxelFlattenResult()
    for k in VoxelFlattenResult.__slots__:
        shape, dtype = shapes[k]
        t = None if out is None else getattr(out, k)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            raise ValueError("out: %s must be a contiguous %s tensor %s on the voxel map's device" % (k, str(dtype).replace("torch.", ""), list(shape)))
        setattr(res, k, t)
    flat = _occupancy_map_struct(words)
    with torch.cuda.device(dev):
        rc = voxel_flatten_lib().sv_voxel_flatten_device(buf.data_ptr(), nbytes, ctypes.byref(vspec), ctypes.byref(flat), ctypes.byref(fspec), int(min_n), int(min_rows),
                                                         int(since), res.logodds.data_ptr(), res.last_seen.data_ptr(), res.floor.data_ptr(), res.top.data_ptr(),
                                                         res.cells.data_ptr(), res.stats.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_flatten_device")
    return res


def debug_voxel_flatten(groups=0, stages=0):
    """sv_debug_voxel_flatten: the workgroups of voxel_map_flatten's two table walks at most (0: the call chooses; 1 .. 2048) and the
    kernels a call enqueues (0: all; 1 .. 4: the first that many of clear, walk A, floor, walk B).  Returns the groups before.
    Process-wide; a test and measurement hook."""
    return int(voxel_flatten_lib().sv_debug_voxel_flatten(int(groups), int(stages)))


def voxel_clusters_lib():
    """The library with the signatures of group (W) declared."""
    return _bind("voxel_clusters")


class VoxelClusterResult(_Result):
    """What voxel_map_clusters returns, tensors on the voxel map's device: clusters int64 [R,16] (stereo_vision.sv.VOXEL_CLUSTER_ROW),
    info int64 [8] (stereo_vision.sv.VOXEL_CLUSTER_INFO; members = -1 for an overflowed map), label int32 [slots] - per slot of the
    table the component's row, -1 no member, -2 in a component below min_voxels, -3 in a kept component without a row - and keys, the
    int64 [slots] strided view of the table's key words (valid while the map's buffer is).  rows and workspace are the tensors the call
    wrote through - hand the result back as `out` and nothing is allocated.  sorted: whether clusters are in ascending least key and cut
    behind that order."""
    __slots__ = ("clusters", "info", "label", "keys", "rows", "workspace", "sorted")


def voxel_cluster_spec(spec):
    """-> SvVoxelClusterSpec from a dict of its words (stereo_vision.sv.voxel_cluster_params'), after stereo_vision.sv.voxel_cluster_words'
    checks (ValueError for a bad word)."""
    from .stereo_vision.sv import voxel_cluster_words
    out = SvVoxelClusterSpec()
    for k, v in voxel_cluster_words(spec).items():
        setattr(out, k, v)
    return out


def voxel_map_clusters(buf, params, connectivity=26, min_voxels=1, capacity=1024, mode=0, z_ref=None, h_lo=None, h_hi=None, flat_map=None, floor=None, min_n=1,
                       min_rows=1, since=0, drop=False, sort=True, out=None, spec=None):
    """The connected components of the voxel map in `buf` - the definition of stereo_vision.sv.voxel_map_clusters on the GPU, bit for
    bit (sv_voxel_clusters_device: eight kernels).  connectivity 6, 18 or 26; a component needs min_voxels voxels for a row; capacity
    rows at most (1 .. 65535); mode 0: heights from z_ref (metres; None: the box's floor) in the band h_lo .. h_hi (metres; None: every
    height); mode 1: heights above `floor`, the int32 [rows,cols] floor plane of a voxel_map_flatten on `flat_map` (its words), in the
    band h_lo .. h_hi (None: 0.2 and 2.0 m, the flatten's obstacle voxels) - stereo_vision.sv.voxel_cluster_params; spec: that function's
    dict instead of the words before it.  min_n >= 1, min_rows, since: the read-out's filters.  drop: the members of components below
    min_voxels are emptied - tombstones until the next carry.  out: an earlier VoxelClusterResult of this map whose tensors are written
    again.
    sort=True: the kept count is read back (the one synchronisation); the C entry writes the rows of up to min(65535, the map's
    capacity) kept components in the order of their roots' slots, torch.sort orders them by least key, the cut to `capacity` is made
    behind that, and label is remapped through the inverse permutation: clusters [min(kept, capacity),16] and label equal the numpy
    form's (voxel_cluster_labels) in shape, dtype and bits while the map holds at most 65535 kept components.
    sort=False: what the C entry wrote with `capacity` rows, not waited for: clusters [capacity,16] in the order of the roots' slots -
    which depends on the schedule of the inserts, as does which components are cut -, zero rows behind min(kept, capacity).
    -> VoxelClusterResult; enqueued on torch's current stream; no other work on the map may run on another stream meanwhile."""
    import torch
    from .stereo_vision.sv import VOXEL_CLUSTER_CAPACITY_MAX, VOXEL_CLUSTER_CUT, occupancy_map_words, voxel_cluster_params
    vspec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, vspec)
    dev = buf.device
    words = voxel_cluster_params(params, connectivity, min_voxels, capacity, mode, z_ref, h_lo, h_hi, drop) if spec is None else dict(spec)
    cspec = voxel_cluster_spec(words)
    capacity = cspec.capacity
    for v, what, lo in ((min_n, "min_n", 1), (min_rows, "min_rows", -2 ** 63)):
        if isinstance(v, bool) or int(v) != v or not lo <= v < 2 ** 63:
            raise ValueError("%s must be an integer >= %d, got %r" % (what, lo, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    flat = None
    if cspec.mode == 1:
        if flat_map is None or floor is None:
            raise ValueError("mode 1 needs flat_map and floor: the words and the floor plane of a flatten")
        fw = occupancy_map_words(flat_map)
        if not (isinstance(floor, torch.Tensor) and floor.device == dev and floor.dtype == torch.int32 and tuple(floor.shape) == (fw["rows"], fw["cols"]) and floor.is_contiguous()):
            raise ValueError("floor must be a contiguous int32 tensor [%d,%d] on the voxel map's device" % (fw["rows"], fw["cols"]))
        flat = _occupancy_map_struct(fw)
    L = voxel_clusters_lib()
    slots = int(L.sv_voxel_map_slots(vspec.capacity))
    n_rows = min(VOXEL_CLUSTER_CAPACITY_MAX, max(capacity, vspec.capacity)) if sort else capacity  # sort: the cut is made behind the order
    ws_bytes = int(L.sv_voxel_clusters_workspace_bytes(vspec.capacity, n_rows))
    shapes = {"rows": ((n_rows, 16), torch.int64), "info": ((8,), torch.int64), "label": ((slots,), torch.int32), "workspace": ((ws_bytes // 4,), torch.int32)}
    if out is not None and not isinstance(out, VoxelClusterResult):
        raise ValueError("out must be a VoxelClusterResult")
    res = VoxelClusterResult(sorted=bool(sort))
    for k, (shape, dtype) in shapes.items():
        t = None if out is None else getattr(out, k)
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()):
            t = torch.empty(shape, dtype=dtype, device=dev)  # another map, another capacity or another sort: new tensors
        setattr(res, k, t)
    res.keys = buf[4:].as_strided((slots,), (11,))
    cspec.capacity = n_rows
    with torch.cuda.device(dev):
        rc = L.sv_voxel_clusters_device(buf.data_ptr(), nbytes, ctypes.byref(vspec), ctypes.byref(cspec), None if flat is None else ctypes.byref(flat),
                                        None if flat is None else floor.data_ptr(), int(min_n), int(min_rows), int(since), res.label.data_ptr(), res.rows.data_ptr(),
                                        res.info.data_ptr(), res.workspace.data_ptr(), ws_bytes, torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_clusters_device")
    if not sort:
        res.clusters = res.rows
        return res
    written = min(max(int(res.info[2]), 0), n_rows)  # the synchronisation
    order = torch.sort(res.rows[:written, 0]).indices
    res.clusters = res.rows[:written][order][:capacity].contiguous()
    rank = torch.empty((written + 3,), dtype=torch.int32, device=dev)  # the inverse permutation, and -3, -2, -1 onto themselves behind it
    rank[order] = torch.arange(written, dtype=torch.int32, device=dev)
    rank[:written][rank[:written] >= capacity] = VOXEL_CLUSTER_CUT
    rank[written:] = torch.tensor([-3, -2, -1], dtype=torch.int32, device=dev)
    res.label = rank[res.label.long()]  # a negative label indexes from the end
    return res


def voxel_cluster_labels(result):
    """-> (key, cluster) of the slots that hold a key, ordered by key: an int64 and an int32 tensor on the map's device, what
    stereo_vision.sv.voxel_map_clusters returns as "key" and "label".  Reads the number of such slots back: this synchronises.  Call
    it before anything else changes the map's keys."""
    import torch
    at = torch.nonzero(result.keys != -1).reshape(-1)
    order = torch.sort(result.keys[at]).indices
    return result.keys[at][order], result.label[at][order]


def voxel_cluster_boxes(result, params):
    """The rows of a VoxelClusterResult (or an int64 [R,16] tensor or array of them) in metres, in double on the host:
    stereo_vision.sv.voxel_cluster_boxes' dict of numpy arrays - centre, lo, hi [R,3], key, voxels, n, first_seq, last_seq [R].  Rows
    without voxels - the zero rows behind the kept ones of sort=False - are left out.  Reads the rows back."""
    import torch
    from .stereo_vision import sv
    rows = result.clusters if isinstance(result, VoxelClusterResult) else result
    rows = rows.cpu().numpy() if isinstance(rows, torch.Tensor) else np.asarray(rows)
    rows = rows.reshape(-1, 16)
    return sv.voxel_cluster_boxes(rows[rows[:, 1] > 0], params)


def debug_voxel_clusters(groups=0, stages=0):
    """sv_debug_voxel_clusters: the workgroups of voxel_map_clusters' table walks at most (0: the call chooses; 1 .. 2048) and `stages`:
    the low four bits the kernels a call enqueues (0: all; 1 .. 7: the first that many of init, link, roots, count, scan, rank, stats),
    16: no combining of equal destinations over the wavefront, 32: no path compression in the link kernel.  Returns the groups before.
    Process-wide; a test and measurement hook."""
    return int(voxel_clusters_lib().sv_debug_voxel_clusters(int(groups), int(stages)))


def voxel_align_lib():
    """The library with the signatures of group (X) declared."""
    return _bind("voxel_align")


class VoxelAlignResult(_Result):
    """What voxel_map_align_sums returns, tensors on the map's device: sums int64 [B,19] (stereo_vision.sv.VOXEL_ALIGN_SUMS names the
    words), pair_key int64 [B,cap] and pair_d2 int32 [B,cap] (both None where not asked for).  voxel_map_align fills the rest, host
    numpy: poses float64 [B,12], ok bool [B], rounds, pairs int64 [rounds,B], rms float64 [rounds,B]."""
    __slots__ = ("sums", "pair_key", "pair_d2", "poses", "ok", "rounds", "pairs", "rms")


def _voxel_align_frames(buf, params, xyz, n, counts, min_n, min_rows, since):
    """The checks of a frame batch that voxel_map_align_sums and voxel_map_align share -> (spec, the map's bytes, xyz, n, counts), the
    tensors contiguous."""
    import torch
    spec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, spec)
    dev = buf.device
    if not (isinstance(xyz, torch.Tensor) and xyz.device == dev and xyz.dtype in (torch.float32, torch.float64) and xyz.dim() == 3 and xyz.shape[2] == 3):
        raise ValueError("xyz must be a float32 or float64 tensor [B,cap,3] on the map's device")
    B, cap = int(xyz.shape[0]), int(xyz.shape[1])
    for t, name, dtype, shape in ((n, "n", torch.int32, (B, cap)), (counts, "counts", torch.int32, (B,))):
        if t is None and name != "counts":
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape):
            raise ValueError("%s must be a %s tensor %s on the map's device" % (name, str(dtype).replace("torch.", ""), list(shape)))
    if B > 65535:
        raise ValueError("at most 65535 frames per call, got %d" % B)
    for v, what in ((min_n, "min_n"), (min_rows, "min_rows")):
        if isinstance(v, bool) or int(v) != v or not -2 ** 63 <= v < 2 ** 63:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    return spec, nbytes, xyz.contiguous(), None if n is None else n.contiguous(), counts.contiguous()


def _voxel_align_origin(origin, B, dev):
    """origin as a contiguous int32 [B,3] tensor on dev: a numpy array of integers within +-2^30 - uploaded once - or such a tensor."""
    import torch
    if isinstance(origin, torch.Tensor):
        if origin.device != dev or origin.dtype != torch.int32 or tuple(origin.shape) != (B, 3):
            raise ValueError("origin must be an int32 tensor [%d,3] on the device (%s) of the map" % (B, dev))
        return origin.contiguous()
    o = np.asarray(origin)
    if o.shape != (B, 3) or o.dtype.kind not in "iu" or (np.abs(o.astype(np.int64)) > 2 ** 30).any():
        raise ValueError("origin must be integers [%d,3] within +-2^30, got %s %s" % (B, o.dtype, o.shape))
    return torch.from_numpy(np.ascontiguousarray(o, dtype=np.int32)).to(dev)


def voxel_map_align_sums(buf, params, xyz, n, counts, poses, origin, max_dist=1.0, min_n=1, min_rows=1, since=0, want_rows=False, out=None, workspace=None):
    """The rows of B frames - xyz CUDA float32 or float64 [B,cap,3], n int32 [B,cap] or None, counts int32 [B], as voxel_map_insert takes
    them -, each under its one pose (float64 [B,12] or [B,4]; numpy or a tensor on the map's device), paired with the nearest voxel
    means of the map in `buf`, and the pairs' sums about origin (integers [B,3] in 1/256 of a cell from lo,
    stereo_vision.sv.voxel_align_origin; numpy or an int32 tensor on the device): the definition of
    stereo_vision.sv.voxel_map_align_sums on the GPU, bit for bit (sv_voxel_align_device: two kernels, no atomics).  max_dist in cells;
    min_n, min_rows and since are the read-out's filters.  want_rows=True also returns the nearest voxel's key and d2 per row.  out: a
    VoxelAlignResult of an earlier call of the same shape to write into; workspace: an int64 tensor to use (None: torch's allocator,
    which keeps it for the next call of the shape).  The map is not changed and nothing is read back.  -> VoxelAlignResult; enqueued on
    torch's current stream, not waited for."""
    import torch
    from .stereo_vision.sv import voxel_align_max_d2
    max_d2 = voxel_align_max_d2(max_dist)
    spec, nbytes, xyz, n, counts = _voxel_align_frames(buf, params, xyz, n, counts, min_n, min_rows, since)
    dev = buf.device
    B, cap = int(xyz.shape[0]), int(xyz.shape[1])
    p = voxel_map_poses(poses, dev)
    if p.shape[0] != B:
        raise ValueError("poses must hold one pose per frame: %d, got %d" % (B, p.shape[0]))
    o = _voxel_align_origin(origin, B, dev)
    res = out if out is not None else VoxelAlignResult(sums=torch.empty((B, 19), dtype=torch.int64, device=dev))
    if want_rows and res.pair_key is None:
        res.pair_key, res.pair_d2 = torch.empty((B, cap), dtype=torch.int64, device=dev), torch.empty((B, cap), dtype=torch.int32, device=dev)
    if tuple(res.sums.shape) != (B, 19) or (want_rows and tuple(res.pair_key.shape) != (B, cap)):
        raise ValueError("out is of another shape")
    if B == 0:  # nothing to enqueue
        return res
    L = voxel_align_lib()
    need = ctypes.c_size_t()
    _check(L.sv_voxel_align_workspace(cap, B, ctypes.byref(need)), "sv_voxel_align_workspace")
    ws = workspace if workspace is not None else torch.empty((max(need.value // 8, 1),), dtype=torch.int64, device=dev)
    rows = [res.pair_key, res.pair_d2] if want_rows else [None, None]
    with torch.cuda.device(dev):
        rc = L.sv_voxel_align_device(buf.data_ptr(), nbytes, ctypes.byref(spec), _ptr(xyz), 0 if xyz.dtype == torch.float32 else 1, _ptr(n), counts.data_ptr(),
                                     p.data_ptr(), o.data_ptr(), B, cap, max_d2, int(min_n), int(min_rows), int(since), res.sums.data_ptr(),
                                     *[None if t is None else t.data_ptr() for t in rows], ws.data_ptr(), ws.numel() * 8, torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_align_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def voxel_map_align(buf, params, xyz, n, counts, poses, iterations=10, max_dist=1.0, dof=6, min_pairs=6, eps=None, min_n=1, min_rows=1, since=0, method="point",
                    normals=None):
    """Iterative closest point of B frames against the map in `buf` - stereo_vision.sv.voxel_map_align with the sums from the device: per
    round the origin from the current poses, voxel_map_align_sums, the B x 19 words read back - the stage's one wait, once per round -
    and stereo_vision.sv.voxel_align_solve on them, until every fitted frame's step is below eps or `iterations` rounds are done.  The
    fit and the loop are the numpy definition's own functions on equal sums, so the poses, ok, rounds, pairs and rms equal the CPU
    path's bit for bit.  poses: the start, float64 [B,12] or [B,4], numpy or a tensor.  -> VoxelAlignResult with sums (the last round's,
    on the device), poses float64 numpy [B,12], ok, rounds, pairs and rms.  eps None: (1e-5, 1 / 256), and
    stereo_vision.sv.VOXEL_ALIGN_PLANE_EPS for the planes.
    method="plane": the point-to-plane rounds of group (Y) - voxel_map_align_plane_sums, B x 32 words read back per round, and
    stereo_vision.sv.voxel_align_solve_plane -> VoxelPlaneResult.  normals: a VoxelNormalsResult of this map (None: voxel_map_normals with
    its defaults and these filters, one kernel more in front of the loop)."""
    import torch
    from .stereo_vision.sv import VOXEL_ALIGN_METHODS, VOXEL_ALIGN_PLANE_EPS, voxel_align_loop, voxel_align_max_d2, voxel_align_plane_solver, voxel_map_pose_words
    voxel_align_max_d2(max_dist)
    if method not in VOXEL_ALIGN_METHODS:
        raise ValueError("method must be 'point' or 'plane', got %r" % (method,))
    if method == "point" and normals is not None:
        raise ValueError("normals go with method='plane'")
    _, _, xyz, n, counts = _voxel_align_frames(buf, params, xyz, n, counts, min_n, min_rows, since)
    B = int(xyz.shape[0])
    start = voxel_map_pose_words(poses.cpu().numpy() if isinstance(poses, torch.Tensor) else poses) if B else np.zeros((0, 12))
    if start.shape[0] != B:
        raise ValueError("poses must hold one pose per frame: %d, got %d" % (B, start.shape[0]))
    if method == "plane":
        if normals is None:
            normals = voxel_map_normals(buf, params, None, min_n=min_n, min_rows=min_rows, since=since)
        elif not isinstance(normals, VoxelNormalsResult):
            raise ValueError("normals must be a VoxelNormalsResult of this map")
        res = VoxelPlaneResult(sums=torch.zeros((B, 32), dtype=torch.int64, device=buf.device))

        def plane_sums_of(cur, origin):
            voxel_map_align_plane_sums(buf, params, xyz, n, counts, cur, origin, normals, max_dist, min_n, min_rows, since, out=res)
            return res.sums.cpu().numpy()  # the wait of the round

        got = voxel_align_loop(plane_sums_of, params, start, iterations, dof, min_pairs, VOXEL_ALIGN_PLANE_EPS if eps is None else eps,
                               voxel_align_plane_solver(normals.dirs.cpu().numpy()))
        res.poses, res.ok, res.rounds, res.pairs, res.rms = got["poses"], got["ok"], got["rounds"], got["pairs"], got["rms"]
        return res
    res = VoxelAlignResult(sums=torch.zeros((B, 19), dtype=torch.int64, device=buf.device))

    def sums_of(cur, origin):
        voxel_map_align_sums(buf, params, xyz, n, counts, cur, origin, max_dist, min_n, min_rows, since, out=res)
        return res.sums.cpu().numpy()  # the wait of the round

    got = voxel_align_loop(sums_of, params, start, iterations, dof, min_pairs, (1e-5, 1.0 / 256) if eps is None else eps)
    res.poses, res.ok, res.rounds, res.pairs, res.rms = got["poses"], got["ok"], got["rounds"], got["pairs"], got["rms"]
    return res


def debug_voxel_align(max_chunks=0, skip=True):
    """sv_debug_voxel_align: the chunks of rows per frame at most (0: the default, 512; 1 .. 512 lowers it, so that a workgroup takes
    several chunks) and whether the score kernel leaves out the cells that cannot hold the nearest voxel.  The results depend on
    neither.  Process-wide; a test and measurement hook."""
    return int(voxel_align_lib().sv_debug_voxel_align(int(max_chunks), 0 if skip else 1))


def voxel_normals_lib():
    """The library with the signatures of group (Y) declared."""
    return _bind("voxel_normals")


class VoxelNormalsResult(_Result):
    """What voxel_map_normals returns, tensors on the map's device: normal int32 [slots] (the index of a direction of `dirs`, -1 for none
    and for every slot that is no member), fit int64 [slots,4] (N, lam1, lam2, lam3 of a member; None where not asked for), counts int64
    [4] (stereo_vision.sv.VOXEL_NORMAL_COUNTS), dirs int8 [K,4] - the table, uploaded once -, and keys, a view of the map's key words."""
    __slots__ = ("normal", "fit", "counts", "dirs", "keys")


class VoxelPlaneResult(_Result):
    """What voxel_map_align_plane_sums returns, tensors on the map's device: sums int64 [B,32] (stereo_vision.sv.VOXEL_PLANE_SUMS names the
    words), pair_key int64, pair_d2 and pair_normal int32 [B,cap] (None where not asked for).  voxel_map_align(method="plane") fills the
    rest, host numpy: poses float64 [B,12], ok bool [B], rounds, pairs int64 [rounds,B] - the plane pairs -, rms float64 [rounds,B]."""
    __slots__ = ("sums", "pair_key", "pair_d2", "pair_normal", "poses", "ok", "rounds", "pairs", "rms")


def voxel_normal_table(dirs, dev):
    """A table of directions as a contiguous int8 [K,4] tensor on dev, 1 <= K <= 4096: a numpy array (stereo_vision.sv.voxel_normal_dirs')
    is uploaded once, a tensor is checked."""
    import torch
    if isinstance(dirs, torch.Tensor):
        if dirs.device != dev or dirs.dtype != torch.int8 or dirs.dim() != 2 or dirs.shape[1] != 4 or not 1 <= dirs.shape[0] <= 4096:
            raise ValueError("dirs must be an int8 tensor [K,4] with 1 <= K <= 4096 on the device (%s) of the map" % (dev,))
        return dirs.contiguous()
    d = np.asarray(dirs)
    if d.dtype != np.int8 or d.ndim != 2 or d.shape[1] != 4 or not 1 <= d.shape[0] <= 4096:
        raise ValueError("dirs must be int8 [K,4] with 1 <= K <= 4096, got %s %s" % (d.dtype, d.shape))
    return torch.from_numpy(np.ascontiguousarray(d)).to(dev)


def voxel_map_normals(buf, params, dirs=None, min_nb=5, flat=64, wide=16, min_n=1, min_rows=1, since=0, want_fit=False, out=None):
    """The surface normals of the voxels of the map in `buf`: the definition of stereo_vision.sv.voxel_map_normals on the GPU, bit for bit
    (sv_voxel_normals_device: one kernel, a lane per slot).  dirs: the table of directions, int8 [K,4], numpy or a tensor on the map's
    device (None: stereo_vision.sv.voxel_normal_dirs()); min_nb in 3 .. 27, flat and wide in 0 .. 256; min_n, min_rows and since are the
    read-out's filters.  want_fit=True also returns N, lam1, lam2, lam3 per slot.  out: a VoxelNormalsResult of an earlier call on a map
    of the same capacity to write into.  The map is not changed and nothing is read back.  -> VoxelNormalsResult, per SLOT - the numpy
    form answers per entry in ascending key; voxel_normal_labels orders this one so -; enqueued on torch's current stream, not waited for."""
    import torch
    from .stereo_vision import sv
    sv._voxel_normal_words(min_nb, flat, wide)
    spec = voxel_map_spec(params)
    nbytes = _voxel_map_buffer(buf, spec)
    dev = buf.device
    for v, what in ((min_n, "min_n"), (min_rows, "min_rows")):
        if isinstance(v, bool) or int(v) != v or not -2 ** 63 <= v < 2 ** 63:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    if isinstance(since, bool) or int(since) != since or not -2 ** 31 <= since < 2 ** 31:
        raise ValueError("since must be a 32-bit integer, got %r" % (since,))
    table = voxel_normal_table(sv.voxel_normal_dirs() if dirs is None else dirs, dev)
    slots = sv.voxel_map_slots(spec.capacity)
    res = out if out is not None else VoxelNormalsResult(normal=torch.empty((slots,), dtype=torch.int32, device=dev), counts=torch.empty((4,), dtype=torch.int64, device=dev))
    if want_fit and res.fit is None:
        res.fit = torch.empty((slots, 4), dtype=torch.int64, device=dev)
    if tuple(res.normal.shape) != (slots,) or res.normal.device != dev:
        raise ValueError("out is of another map's shape")
    res.dirs, res.keys = table, buf[4:].as_strided((slots,), (11,))
    with torch.cuda.device(dev):
        rc = voxel_normals_lib().sv_voxel_normals_device(buf.data_ptr(), nbytes, ctypes.byref(spec), table.data_ptr(), int(table.shape[0]), int(min_nb), int(flat), int(wide),
                                                         int(min_n), int(min_rows), int(since), res.normal.data_ptr(), slots, res.fit.data_ptr() if want_fit else None,
                                                         res.counts.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_normals_device")
    return res


def voxel_normal_labels(result):
    """-> (key, normal, fit or None) of the slots that hold a key, ordered by key: what stereo_vision.sv.voxel_map_normals returns as
    "key", "normal" and "fit".  Reads the number of such slots back: this synchronises.  Call it before anything else changes the map's
    keys."""
    import torch
    at = torch.nonzero(result.keys != -1).reshape(-1)
    at = at[torch.sort(result.keys[at]).indices]
    return result.keys[at], result.normal[at], None if result.fit is None else result.fit[at]


def voxel_map_align_plane_sums(buf, params, xyz, n, counts, poses, origin, normals, max_dist=1.0, min_n=1, min_rows=1, since=0, want_rows=False, out=None, workspace=None):
    """The sums of one round of point-to-plane alignment: the definition of stereo_vision.sv.voxel_map_align_plane_sums on the GPU, bit for
    bit (sv_voxel_plane_align_device: two kernels, no atomics).  Every argument of voxel_map_align_sums means here what it means there;
    normals is a VoxelNormalsResult of this map - its per-slot normal and its table are taken as they are -, or a pair (normal int32
    [slots] tensor, dirs).  want_rows=True also returns pair_key, pair_d2 and pair_normal per row.  -> VoxelPlaneResult; enqueued on
    torch's current stream, not waited for."""
    import torch
    from .stereo_vision.sv import voxel_align_max_d2, voxel_map_slots
    max_d2 = voxel_align_max_d2(max_dist)
    spec, nbytes, xyz, n, counts = _voxel_align_frames(buf, params, xyz, n, counts, min_n, min_rows, since)
    dev = buf.device
    B, cap = int(xyz.shape[0]), int(xyz.shape[1])
    normal, dirs = (normals.normal, normals.dirs) if isinstance(normals, VoxelNormalsResult) else normals
    table = voxel_normal_table(dirs, dev)
    slots = voxel_map_slots(spec.capacity)
    if not (isinstance(normal, torch.Tensor) and normal.device == dev and normal.dtype == torch.int32 and tuple(normal.shape) == (slots,)):
        raise ValueError("normal must be an int32 tensor [%d], one word per slot, on the map's device" % slots)
    normal = normal.contiguous()
    p = voxel_map_poses(poses, dev)
    if p.shape[0] != B:
        raise ValueError("poses must hold one pose per frame: %d, got %d" % (B, p.shape[0]))
    o = _voxel_align_origin(origin, B, dev)
    res = out if out is not None else VoxelPlaneResult(sums=torch.empty((B, 32), dtype=torch.int64, device=dev))
    if want_rows and res.pair_key is None:
        res.pair_key = torch.empty((B, cap), dtype=torch.int64, device=dev)
        res.pair_d2, res.pair_normal = torch.empty((B, cap), dtype=torch.int32, device=dev), torch.empty((B, cap), dtype=torch.int32, device=dev)
    if tuple(res.sums.shape) != (B, 32) or (want_rows and tuple(res.pair_key.shape) != (B, cap)):
        raise ValueError("out is of another shape")
    if B == 0:  # nothing to enqueue
        return res
    L = voxel_normals_lib()
    need = ctypes.c_size_t()
    _check(L.sv_voxel_plane_align_workspace(cap, B, ctypes.byref(need)), "sv_voxel_plane_align_workspace")
    ws = workspace if workspace is not None else torch.empty((max(need.value // 8, 1),), dtype=torch.int64, device=dev)
    rows = [res.pair_key, res.pair_d2, res.pair_normal] if want_rows else [None, None, None]
    with torch.cuda.device(dev):
        rc = L.sv_voxel_plane_align_device(buf.data_ptr(), nbytes, ctypes.byref(spec), _ptr(xyz), 0 if xyz.dtype == torch.float32 else 1, _ptr(n), counts.data_ptr(),
                                           p.data_ptr(), o.data_ptr(), B, cap, max_d2, int(min_n), int(min_rows), int(since), normal.data_ptr(), slots, table.data_ptr(),
                                           int(table.shape[0]), res.sums.data_ptr(), *[None if t is None else t.data_ptr() for t in rows], ws.data_ptr(), ws.numel() * 8,
                                           torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_voxel_plane_align_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def debug_voxel_normals(max_chunks=0, skip=True, prune=True):
    """sv_debug_voxel_normals: the chunks of rows per frame at most of the plane score kernel (0: the default, 512), whether it leaves out
    the cells that cannot hold the nearest voxel, and whether the normals kernel leaves out the search of a member with N < min_nb where
    no fit is asked for.  The results depend on none of them.  Process-wide; a test and measurement hook."""
    return int(voxel_normals_lib().sv_debug_voxel_normals(int(max_chunks), (0 if skip else 1) | (0 if prune else 2)))


def flow_lib():
    """The library with the signatures of group (Z) declared."""
    return _bind("flow")


class FlowResult(_Result):
    """What flow_match returns, tensors on the images' device: matches int32 [B,capacity,6] = (u0, v0, d0q, u1, v1, d1q), cost int32
    [B,capacity,2] = (best, second), counts int32 [B] (-1: more matches than capacity).  flow_egomotion's result has sums int64 [B,32] on
    the device and, host numpy, poses float64 [B,12], ok bool [B], rounds, inliers int64 [rounds,B], rms_px float64 [rounds,B]."""
    __slots__ = ("matches", "cost", "counts", "sums", "poses", "ok", "rounds", "inliers", "rms_px")


def flow_spec(camera, **words):
    """-> SvFlowSpec from a camera dict (stereo_vision.sv.voxel_render_camera's) and flow_match's words (stereo_vision.sv.flow_words checks
    them: ValueError)."""
    from .stereo_vision.sv import flow_camera, flow_words
    cam, w = flow_camera(camera), flow_words(**words)
    return SvFlowSpec(cam["f"], cam["cx"], cam["cy"], cam["b16"], cam["fb"], cam["fb16"], w["step"], w["r"], w["wx"], w["wy"], w["ratio"], w["max_cost"], w["capacity"])


def flow_match(prev, cur, d_prev, d_cur, camera, guess=None, step=8, r=4, wx=8, wy=8, ratio=230, max_cost=225 * 255, capacity=4096, out=None, workspace=None):
    """Temporal matches of B frame pairs - the definition of stereo_vision.sv.flow_match on the GPU, bit for bit (sv_flow_match_device: a
    wavefront per lattice point with its window of cur in LDS, four bytes per v_sad_u8; then the matches packed in point order; no
    atomics).  prev, cur CUDA uint8 [B,H,W]: the rectified left gray images of frames k - 1 and k (StereoRig.frontend's); d_prev CUDA
    float32 [B,H,W]: the disparity of frame k - 1; d_cur the same of frame k, or None; camera: voxel_render_camera's dict; guess float64
    [B,12] (numpy, or a tensor on the device) or None: the expected motion, previous camera to current camera.  out: a FlowResult of an
    earlier call of the same shape to write into; workspace: an int32 tensor to use (None: torch's allocator).  -> FlowResult(matches,
    cost, counts); enqueued on torch's current stream, nothing is read back."""
    import torch
    spec = flow_spec(camera, step=step, r=r, wx=wx, wy=wy, ratio=ratio, max_cost=max_cost, capacity=capacity)
    if not (isinstance(prev, torch.Tensor) and prev.is_cuda and prev.dtype == torch.uint8 and prev.dim() == 3):
        raise ValueError("prev must be a CUDA uint8 tensor [B,H,W]")
    dev, shape = prev.device, tuple(prev.shape)
    B, H, W = shape
    if B > 65535 or not (1 <= H <= 8192 and 1 <= W <= 8192):
        raise ValueError("at most 65535 frames of at most 8192 x 8192, got %s" % (shape,))
    for t, name, dtype in ((cur, "cur", torch.uint8), (d_prev, "d_prev", torch.float32), (d_cur, "d_cur", torch.float32)):
        if t is None and name == "d_cur":
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape):
            raise ValueError("%s must be a %s tensor %s on %s" % (name, str(dtype).replace("torch.", ""), list(shape), dev))
    prev, cur, d_prev = prev.contiguous(), cur.contiguous(), d_prev.contiguous()
    d_cur = None if d_cur is None else d_cur.contiguous()
    g = None
    if guess is not None:
        g = guess if isinstance(guess, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(guess, np.float64)).to(dev)
        if g.device != dev or g.dtype != torch.float64 or tuple(g.shape) != (B, 12):
            raise ValueError("guess must be float64 [%d,12]" % B)
        g = g.contiguous()
    cap = int(capacity)
    res = out if out is not None else FlowResult(matches=torch.empty((B, cap, 6), dtype=torch.int32, device=dev), cost=torch.empty((B, cap, 2), dtype=torch.int32, device=dev),
                                                 counts=torch.empty((B,), dtype=torch.int32, device=dev))
    if tuple(res.matches.shape) != (B, cap, 6) or tuple(res.cost.shape) != (B, cap, 2) or tuple(res.counts.shape) != (B,):
        raise ValueError("out is of another shape")
    L = flow_lib()
    need = ctypes.c_size_t()
    _check(L.sv_flow_match_workspace(W, H, B, ctypes.byref(spec), ctypes.byref(need)), "sv_flow_match_workspace")
    if B == 0:  # nothing to enqueue
        return res
    ws = workspace if workspace is not None else torch.empty((max(need.value // 4, 1),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.sv_flow_match_device(prev.data_ptr(), cur.data_ptr(), d_prev.data_ptr(), None if d_cur is None else d_cur.data_ptr(), None if g is None else g.data_ptr(),
                                    B, W, H, ctypes.byref(spec), _ptr(res.matches), _ptr(res.cost), res.counts.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                    torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_flow_match_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def _flow_matches(matches, counts):
    import torch
    if not (isinstance(matches, torch.Tensor) and matches.is_cuda and matches.dtype == torch.int32 and matches.dim() == 3 and matches.shape[2] == 6):
        raise ValueError("matches must be a CUDA int32 tensor [B,capacity,6]")
    B, cap = int(matches.shape[0]), int(matches.shape[1])
    if B > 65535 or cap > 65536:
        raise ValueError("at most 65535 frames of at most 65536 matches, got %s" % (tuple(matches.shape),))
    if not (isinstance(counts, torch.Tensor) and counts.device == matches.device and counts.dtype == torch.int32 and tuple(counts.shape) == (B,)):
        raise ValueError("counts must be an int32 tensor [%d] on the device of matches" % B)
    return matches.contiguous(), counts.contiguous(), B, cap


def flow_pose_sums(matches, counts, camera, poses, gate_q=None, dgate_q=None, out=None, workspace=None):
    """The sums of one round of the egomotion fit - the definition of stereo_vision.sv.flow_pose_sums on the GPU, bit for bit
    (sv_flow_pose_sums_device: a lane per match, two kernels, no atomics).  matches CUDA int32 [B,capacity,6] and counts int32 [B] as
    flow_match returns them, poses float64 [B,12] (numpy, or a tensor on the device), gate_q and dgate_q in 1/16 px (None: 2^20, no
    gate).  out: an int64 [B,32] tensor to write into.  -> int64 [B,32] on the device; enqueued on torch's current stream, nothing is
    read back."""
    import torch
    from .stereo_vision.sv import _flow_gates
    gate_q, dgate_q = _flow_gates(gate_q, dgate_q)
    spec = flow_spec(camera)
    matches, counts, B, cap = _flow_matches(matches, counts)
    dev = matches.device
    p = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poses, np.float64)).to(dev)
    if p.device != dev or p.dtype != torch.float64 or tuple(p.shape) != (B, 12):
        raise ValueError("poses must be float64 [%d,12]" % B)
    p = p.contiguous()
    sums = out if out is not None else torch.empty((B, 32), dtype=torch.int64, device=dev)
    if tuple(sums.shape) != (B, 32) or sums.dtype != torch.int64 or sums.device != dev or not sums.is_contiguous():
        raise ValueError("out must be a contiguous int64 tensor [%d,32] on the device of matches" % B)
    if B == 0:
        return sums
    L = flow_lib()
    need = ctypes.c_size_t()
    _check(L.sv_flow_pose_sums_workspace(cap, B, ctypes.byref(need)), "sv_flow_pose_sums_workspace")
    ws = workspace if workspace is not None else torch.empty((max(need.value // 8, 1),), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.sv_flow_pose_sums_device(_ptr(matches), counts.data_ptr(), p.data_ptr(), B, cap, ctypes.byref(spec), gate_q, dgate_q, sums.data_ptr(), ws.data_ptr(),
                                        ws.numel() * 8, torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_flow_pose_sums_device")
    return sums


def flow_egomotion(matches, counts, camera, start=None, gates=None, dgate=2.0, iterations=10, eps=None, min_inliers=12):
    """The camera's motion between two frames from their matches - stereo_vision.sv.flow_egomotion with the sums from the device: per
    round flow_pose_sums and the B x 32 words read back - the stage's one wait, once per round -, then stereo_vision.sv.flow_solve on
    them.  The fit and the loop are the numpy definition's own functions on equal sums, so the result equals the CPU path's bit for bit.
    -> FlowResult with sums (the last round's, on the device), poses float64 numpy [B,12], ok, rounds, inliers and rms_px."""
    import torch
    from .stereo_vision.sv import FLOW_GATES, flow_identity, flow_loop
    matches, counts, B, _ = _flow_matches(matches, counts)
    start = flow_identity(B) if start is None else np.asarray(start.cpu().numpy() if isinstance(start, torch.Tensor) else start, np.float64)
    if start.shape != (B, 12):
        raise ValueError("start must be float64 [%d,12], got %s" % (B, start.shape))
    res = FlowResult(matches=matches, counts=counts, sums=torch.zeros((B, 32), dtype=torch.int64, device=matches.device))

    def sums_of(cur, gate_q, dgate_q):
        flow_pose_sums(matches, counts, camera, cur, gate_q, dgate_q, out=res.sums)
        return res.sums.cpu().numpy()  # the wait of the round

    got = flow_loop(sums_of, start, FLOW_GATES if gates is None else gates, dgate, iterations, eps, min_inliers)
    res.poses, res.ok, res.rounds, res.inliers, res.rms_px = got["poses"], got["ok"], got["rounds"], got["inliers"], got["rms_px"]
    return res


def warp_lib():
    """The library with the signatures of group (AA) declared."""
    return _bind("warp")


class WarpResult(_Result):
    """What disparity_warp returns, tensors on the inputs' device (numpy arrays for CPU inputs): expected int32 [B,H,W], source int32
    [B,H,W], counts int32 [B,8] (stereo_vision.sv.WARP_COUNTS) and, with a d_cur, label uint8 [B,H,W] (stereo_vision.sv.VOXEL_RENDER_LABELS)
    and out float32 [B,H,W] - None without one."""
    __slots__ = ("expected", "source", "label", "out", "counts")


def warp_spec(camera, **words):
    """-> SvWarpSpec from a camera dict (stereo_vision.sv.voxel_render_camera's) and disparity_warp's words (stereo_vision.sv.warp_words
    checks them: ValueError)."""
    from .stereo_vision.sv import flow_camera, warp_words
    cam, w = flow_camera(camera), warp_words(**words)
    return SvWarpSpec(cam["f"], cam["cx"], cam["cy"], cam["b16"], cam["fb"], cam["fb16"], w["e_max"], w["tol_q"], w["rel_q"], w["mode"])


def disparity_warp(d_prev, d_cur, camera, poses, e_max=1, tol_q=16, rel_q=0, mode="fill", out=None, workspace=None):
    """The disparity maps of frames k - 1 warped into frames k under the motions `poses` and compared with d_cur - the definition of
    stereo_vision.sv.disparity_warp on the GPU, bit for bit (sv_disparity_warp_device: the keys cleared, a lane per source pixel with one
    64-bit integer atomicMax per covered pixel, a lane per target pixel; no float atomics).  d_prev float32 [B,H,W]; d_cur the same or
    None; camera: voxel_render_camera's dict; poses float64 [B,12] (numpy, or a tensor on the device): previous camera to current camera.
    out: a WarpResult of an earlier call of the same shape to write into; workspace: an int64 tensor of B H W words to use (None: torch's
    allocator).  -> WarpResult; for CUDA tensors enqueued on torch's current stream, nothing is read back.  CPU tensors (or numpy
    arrays) run the numpy form and give numpy arrays."""
    import torch
    spec = warp_spec(camera, e_max=e_max, tol_q=tol_q, rel_q=rel_q, mode=mode)
    if not (isinstance(d_prev, torch.Tensor) and d_prev.is_cuda):
        from .stereo_vision.sv import disparity_warp as on_host
        as_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t
        return WarpResult(**on_host(as_np(d_prev), None if d_cur is None else as_np(d_cur), camera, as_np(poses), e_max, tol_q, rel_q, mode))
    if d_prev.dtype != torch.float32 or d_prev.dim() != 3:
        raise ValueError("d_prev must be a float32 tensor [B,H,W]")
    dev, shape = d_prev.device, tuple(d_prev.shape)
    B, H, W = shape
    if B > 65535 or not (1 <= H <= 8192 and 1 <= W <= 8192):
        raise ValueError("at most 65535 frames of at most 8192 x 8192, got %s" % (shape,))
    if d_cur is not None and not (isinstance(d_cur, torch.Tensor) and d_cur.device == dev and d_cur.dtype == torch.float32 and tuple(d_cur.shape) == shape):
        raise ValueError("d_cur must be None or a float32 tensor %s on %s" % (list(shape), dev))
    d_prev = d_prev.contiguous()
    d_cur = None if d_cur is None else d_cur.contiguous()
    p = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poses, np.float64)).to(dev)
    if p.device != dev or p.dtype != torch.float64 or tuple(p.shape) != (B, 12):
        raise ValueError("poses must be float64 [%d,12]" % B)
    p = p.contiguous()
    res = out
    if res is None:
        res = WarpResult(expected=torch.empty(shape, dtype=torch.int32, device=dev), source=torch.empty(shape, dtype=torch.int32, device=dev),
                         counts=torch.empty((B, 8), dtype=torch.int32, device=dev))
        if d_cur is not None:
            res.label, res.out = torch.empty(shape, dtype=torch.uint8, device=dev), torch.empty(shape, dtype=torch.float32, device=dev)
    for t, name, dtype, want in ((res.expected, "expected", torch.int32, shape), (res.source, "source", torch.int32, shape), (res.counts, "counts", torch.int32, (B, 8)),
                                 (res.label, "label", torch.uint8, shape), (res.out, "out", torch.float32, shape)):
        if t is None and d_cur is None and name in ("label", "out"):
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == want and t.is_contiguous()):
            raise ValueError("out.%s must be a contiguous %s tensor %s on %s" % (name, str(dtype).replace("torch.", ""), list(want), dev))
    L = warp_lib()
    need = ctypes.c_size_t()
    _check(L.sv_disparity_warp_workspace(W, H, B, ctypes.byref(need)), "sv_disparity_warp_workspace")
    if B == 0:  # nothing to enqueue
        return res
    ws = workspace if workspace is not None else torch.empty((max(need.value // 8, 1),), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.sv_disparity_warp_device(d_prev.data_ptr(), None if d_cur is None else d_cur.data_ptr(), p.data_ptr(), B, W, H, ctypes.byref(spec), res.expected.data_ptr(),
                                        res.source.data_ptr(), None if d_cur is None else res.label.data_ptr(), None if d_cur is None else res.out.data_ptr(),
                                        res.counts.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_disparity_warp_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def track_lib():
    """The library with the signatures of group (AB) declared."""
    return _bind("track")


def track_spec(camera, max_boxes, width, height, **words):
    """-> SvTrackSpec from a camera dict (stereo_vision.sv.voxel_render_camera's) and object_links' words (stereo_vision.sv.track_words
    checks them: ValueError)."""
    from .stereo_vision.sv import flow_camera, track_words
    cam, w = flow_camera(camera), track_words(max_boxes, width, height, **words)
    return SvTrackSpec(cam["f"], cam["cx"], cam["cy"], cam["b16"], cam["fb"], cam["fb16"], w["width"], w["height"], w["max_boxes"], w["band_q"], w["min_votes"],
                       w["share"], w["gate_m"])


def object_links(matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1, camera, width, height, band_q=48, min_votes=3, share=128, gate_m=0, centre=None, out=None,
                 workspace=None):
    """The boxes of frames k - 1 linked to those of frames k by the temporal matches that lie in both, and the sums of each linked box's own
    motion - the definition of stereo_vision.sv.object_links on the GPU, bit for bit (sv_object_links_device: four kernels, integer
    atomics only).  matches CUDA int32 [B,capacity,6] and counts int32 [B] as flow_match returns them; poses float64 [B,12] (numpy, or a
    tensor on the device): previous camera to current camera; boxes0 int32 [B,M,4], n0 int32 [B] or None, q0 int32 [B,M] - the boxes of
    frames k - 1, their counts and reference disparities in quarter pixels (objects' info[..., 3], box_positions' stat[..., 2]) -; boxes1,
    n1, q1 the same of frames k; M <= 64; camera: voxel_render_camera's dict; width, height: of the maps; band_q (1/16 px), min_votes,
    share, gate_m (1/1024 m, 0: no gate) and centre int32 [B,M,3] or None as there.  out: the dict of an earlier call of the same shape to
    write into; workspace: an int64 tensor of 2 B capacity words to use (None: torch's allocator).  -> {"votes": int32 [B,M,M+1], "link":
    int32 [B,M,4], "sums": int64 [B,M,16]}; for CUDA tensors enqueued on torch's current stream, nothing is read back.  CPU tensors (or
    numpy arrays) run the numpy form and give numpy arrays."""
    import torch
    if not (isinstance(matches, torch.Tensor) and matches.is_cuda):
        from .stereo_vision.sv import object_links as on_host
        as_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t
        return on_host(*[as_np(t) for t in (matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1)], camera, width, height, band_q, min_votes, share, gate_m, as_np(centre))
    matches, counts, B, cap = _flow_matches(matches, counts)
    dev = matches.device
    if not (isinstance(boxes0, torch.Tensor) and boxes0.device == dev and boxes0.dtype == torch.int32 and boxes0.dim() == 3 and boxes0.shape[0] == B and boxes0.shape[2] == 4):
        raise ValueError("boxes0 must be an int32 tensor [%d,max_boxes,4] on the device of matches" % B)
    M = int(boxes0.shape[1])
    spec = track_spec(camera, M, width, height, band_q=band_q, min_votes=min_votes, share=share, gate_m=gate_m)
    p = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poses, np.float64)).to(dev)
    if p.device != dev or p.dtype != torch.float64 or tuple(p.shape) != (B, 12):
        raise ValueError("poses must be float64 [%d,12]" % B)
    c = None if centre is None else centre if isinstance(centre, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(centre)).to(dev)
    ins = []
    for t, name, want, optional in ((boxes0, "boxes0", (B, M, 4), False), (n0, "n0", (B,), True), (q0, "q0", (B, M), False), (boxes1, "boxes1", (B, M, 4), False),
                                    (n1, "n1", (B,), True), (q1, "q1", (B, M), False), (c, "centre", (B, M, 3), True)):
        if t is None and optional:
            ins.append(None)
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int32 and tuple(t.shape) == want):
            raise ValueError("%s must be %san int32 tensor %s on %s" % (name, "None or " if optional else "", list(want), dev))
        ins.append(t.contiguous())
    boxes0, n0, q0, boxes1, n1, q1, c = ins
    p = p.contiguous()
    res = out if out is not None else {"votes": torch.empty((B, M, M + 1), dtype=torch.int32, device=dev), "link": torch.empty((B, M, 4), dtype=torch.int32, device=dev),
                                       "sums": torch.empty((B, M, 16), dtype=torch.int64, device=dev)}
    for name, dtype, want in (("votes", torch.int32, (B, M, M + 1)), ("link", torch.int32, (B, M, 4)), ("sums", torch.int64, (B, M, 16))):
        t = res.get(name)
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == want and t.is_contiguous()):
            raise ValueError("out[%r] must be a contiguous %s tensor %s on %s" % (name, str(dtype).replace("torch.", ""), list(want), dev))
    L = track_lib()
    need = ctypes.c_size_t()
    _check(L.sv_object_links_workspace(cap, B, ctypes.byref(need)), "sv_object_links_workspace")
    if B == 0 or M == 0:  # nothing to enqueue
        return res
    ws = workspace if workspace is not None else torch.empty((max(need.value // 8, 1),), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.sv_object_links_device(_ptr(matches), counts.data_ptr(), p.data_ptr(), B, cap, boxes0.data_ptr(), None if n0 is None else n0.data_ptr(), q0.data_ptr(),
                                      boxes1.data_ptr(), None if n1 is None else n1.data_ptr(), q1.data_ptr(), None if c is None else c.data_ptr(), ctypes.byref(spec),
                                      res["votes"].data_ptr(), res["link"].data_ptr(), res["sums"].data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size(),
                                      torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_object_links_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def debug_object_links(stop=0):
    """sv_debug_object_links: stop = 1 .. 3 leaves the sums, the link and the votes kernel out, from the end - for timing by difference
    only: what they would have written is undefined.  0 is the default.  Process-wide; a measurement hook."""
    _check(track_lib().sv_debug_object_links(int(stop)), "sv_debug_object_links")


def place_lib():
    """The library with the signatures of group (AC) declared."""
    return _bind("place")


def place_spec(params):
    """-> SvPlaceSpec from place_params' dict (stereo_vision.sv.place_params checks the words again: ValueError)."""
    from .stereo_vision.sv import place_params
    w = place_params(params["r_max"], params["rings"], params["sectors"], params["z_lo"], params["z_hi"], params["r_min"])
    return SvPlaceSpec(w["r_max"], w["z_lo"], w["z_hi"], w["r_min"], w["rings"], w["sectors"])


_place_dirs = {}  # (sectors, device) -> the sector table on the device: made once on the host


def _place_outputs(res, wanted, dev):
    """The tensors of `wanted` = ((name, dtype, shape), ...): new ones, or those of the dict `res` of an earlier call, checked."""
    import torch
    if res is None:
        return {name: torch.empty(shape, dtype=dtype, device=dev) for name, dtype, shape in wanted}
    for name, dtype, shape in wanted:
        t = res.get(name)
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous()):
            raise ValueError("out[%r] must be a contiguous %s tensor %s on %s" % (name, str(dtype).replace("torch.", ""), list(shape), dev))
    return res


def place_descriptor(xyz, n, counts, params, poses=None, out=None, workspace=None):
    """The polar height descriptors of B frames of rows - the definition of stereo_vision.sv.place_descriptor on the GPU, bit for bit
    (sv_place_descriptor_device: three kernels, integer atomics only).  xyz CUDA float32 or float64 [B,cap,3], n int32 [B,cap] or None,
    counts int32 [B]: the rows voxel_map_insert takes; params: place_params' dict; poses float64 [B,12] (numpy, or a tensor on the device) or
    None.  out: the dict of an earlier call of the same shape to write into; workspace: an int32 tensor of B (4 + rings sectors) words to
    use (None: torch's allocator).  -> {"desc": uint8 [B,R,S], "ring": uint8 [B,R], "words": int32 [B,4]}; for CUDA tensors enqueued on
    torch's current stream, nothing is read back.  CPU tensors (or numpy arrays) run the numpy form and give numpy arrays."""
    import torch
    if not (isinstance(xyz, torch.Tensor) and xyz.is_cuda):
        from .stereo_vision.sv import place_descriptor as on_host
        as_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t
        return on_host(as_np(xyz), as_np(n), as_np(counts), params, as_np(poses))
    spec = place_spec(params)
    R, S, dev = spec.rings, spec.sectors, xyz.device
    if not (xyz.dtype in (torch.float32, torch.float64) and xyz.dim() == 3 and xyz.shape[2] == 3):
        raise ValueError("xyz must be a float32 or float64 tensor [B,cap,3]")
    B, cap = int(xyz.shape[0]), int(xyz.shape[1])
    for t, name, shape in ((n, "n", (B, cap)), (counts, "counts", (B,))):
        if t is None and name != "counts":
            continue
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int32 and tuple(t.shape) == shape):
            raise ValueError("%s must be an int32 tensor %s on the device of xyz" % (name, list(shape)))
    p = None
    if poses is not None:
        p = poses if isinstance(poses, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(poses, np.float64)).to(dev)
        if p.device != dev or p.dtype != torch.float64 or tuple(p.shape) != (B, 12):
            raise ValueError("poses must be None or float64 [%d,12]" % B)
        p = p.contiguous()
    res = _place_outputs(out, (("desc", torch.uint8, (B, R, S)), ("ring", torch.uint8, (B, R)), ("words", torch.int32, (B, 4))), dev)
    L = place_lib()
    need = ctypes.c_size_t()
    _check(L.sv_place_descriptor_workspace(B, R, S, ctypes.byref(need)), "sv_place_descriptor_workspace")
    if B == 0:  # nothing to enqueue
        return res
    if (S, dev) not in _place_dirs:
        from .stereo_vision.sv import place_params
        _place_dirs[(S, dev)] = torch.from_numpy(place_params(1.0, 1, S)["dirs"]).to(dev)
    dirs = _place_dirs[(S, dev)]
    xyz, counts = xyz.contiguous(), counts.contiguous()
    n = None if n is None else n.contiguous()
    ws = workspace if workspace is not None else torch.empty((need.value // 4,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.sv_place_descriptor_device(_ptr(xyz), 0 if xyz.dtype == torch.float32 else 1, _ptr(n), counts.data_ptr(), None if p is None else p.data_ptr(), B, cap,
                                          dirs.data_ptr(), ctypes.byref(spec), res["desc"].data_ptr(), res["ring"].data_ptr(), res["words"].data_ptr(), ws.data_ptr(),
                                          ws.numel() * ws.element_size(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_place_descriptor_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def place_match(q_desc, q_words, q_ring, q_seq, k_desc, k_words, k_ring, k_seq, min_gap, ring_gate=-1, max_shift=None, accept=256, want_pair=False, out=None,
                workspace=None):
    """Q query descriptors against K stored ones under every rotation - the definition of stereo_vision.sv.place_match on the GPU, bit
    for bit (sv_place_match_device: two kernels, no atomics).  q_desc CUDA uint8 [Q,R,S], q_words int32 [Q,4], q_ring uint8 [Q,R], q_seq
    int32 [Q] and the same of the K keys, on one device; min_gap, ring_gate, max_shift, accept, want_pair as there.  out: the dict of an
    earlier call of the same shape to write into; workspace: an int32 tensor of 8 Q ceil(K / 64) words to use (None: torch's allocator).
    -> {"best": int32 [Q,4], "counts": int32 [Q,3]} and with want_pair "pair": int32 [Q,K,2]; for CUDA tensors enqueued on torch's current
    stream, nothing is read back.  CPU tensors (or numpy arrays) run the numpy form and give numpy arrays."""
    import torch
    from .stereo_vision import sv as _sv
    if not (isinstance(q_desc, torch.Tensor) and q_desc.is_cuda):
        as_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t
        return _sv.place_match(*[as_np(t) for t in (q_desc, q_words, q_ring, q_seq, k_desc, k_words, k_ring, k_seq)], min_gap, ring_gate, max_shift, accept, want_pair)
    dev = q_desc.device
    if not (q_desc.dtype == torch.uint8 and q_desc.dim() == 3 and isinstance(k_desc, torch.Tensor) and k_desc.device == dev and k_desc.dtype == torch.uint8
            and k_desc.dim() == 3 and tuple(k_desc.shape[1:]) == tuple(q_desc.shape[1:])):
        raise ValueError("q_desc and k_desc must be uint8 tensors [Q,R,S] and [K,R,S] on one device")
    (Q, R, S), K = (int(v) for v in q_desc.shape), int(k_desc.shape[0])
    ins = []
    for t, name, dtype, shape in ((q_desc, "q_desc", torch.uint8, (Q, R, S)), (q_words, "q_words", torch.int32, (Q, 4)), (q_ring, "q_ring", torch.uint8, (Q, R)),
                                  (q_seq, "q_seq", torch.int32, (Q,)), (k_desc, "k_desc", torch.uint8, (K, R, S)), (k_words, "k_words", torch.int32, (K, 4)),
                                  (k_ring, "k_ring", torch.uint8, (K, R)), (k_seq, "k_seq", torch.int32, (K,))):
        if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape):
            raise ValueError("%s must be a %s tensor %s on %s" % (name, str(dtype).replace("torch.", ""), list(shape), dev))
        t = t.contiguous()
        ins.append(t.clone() if t.data_ptr() % 4 and name.endswith("desc") else t)  # the C entry reads a descriptor by dwords
    min_gap, ring_gate = _sv._place_int(min_gap, 0, 2 ** 31 - 1, "min_gap"), _sv._place_int(ring_gate, -1, 2 ** 31 - 1, "ring_gate")
    max_shift = -1 if max_shift is None else _sv._place_int(max_shift, 0, _sv.PLACE_SECTORS_MAX, "max_shift")
    accept = _sv._place_int(accept, 0, _sv.PLACE_ACCEPT_MAX, "accept")
    wanted = (("best", torch.int32, (Q, 4)), ("counts", torch.int32, (Q, 3))) + ((("pair", torch.int32, (Q, K, 2)),) if want_pair else ())
    res = _place_outputs(out, wanted, dev)
    L = place_lib()
    need = ctypes.c_size_t()
    _check(L.sv_place_match_workspace(Q, K, ctypes.byref(need)), "sv_place_match_workspace")
    ws = workspace if workspace is not None else torch.empty((max(need.value // 4, 1),), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = L.sv_place_match_device(*[_ptr(t) for t in ins[:4]], Q, *[_ptr(t) for t in ins[4:]], K, R, S, min_gap, ring_gate, max_shift, accept, _ptr(res["best"]),
                                     _ptr(res["counts"]), _ptr(res["pair"]) if want_pair else None, ws.data_ptr(), ws.numel() * ws.element_size(),
                                     torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_place_match_device")
    return res  # ws goes back to torch's allocator, which hands it out again on this stream only: behind the kernels


def pose_graph_lib():
    """The library with the signatures of group (AE) declared."""
    return _bind("pose_graph")


def _pose_graph_tensor(t, dtype, shape, dev, name):
    """A contiguous tensor of `dtype` and `shape` on dev from a tensor there or a numpy array (uploaded)."""
    import torch
    if not isinstance(t, torch.Tensor):
        try:
            t = torch.from_numpy(np.ascontiguousarray(t, dtype={torch.float64: np.float64, torch.int32: np.int32, torch.uint8: np.uint8}[dtype]).reshape(shape)).to(dev)
        except (TypeError, ValueError):
            raise ValueError("%s must be %s %s" % (name, str(dtype).replace("torch.", ""), list(shape)))
    if t.dtype == torch.bool and dtype == torch.uint8:
        t = t.to(torch.uint8)
    if t.device != dev or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError("%s must be a %s tensor %s on %s" % (name, str(dtype).replace("torch.", ""), list(shape), dev))
    return t.contiguous()


def _pose_graph_spec(lam, tol):
    lam, tol = float(lam), float(tol)
    if not (lam > 0.0 and np.isfinite(lam)):
        raise ValueError("lam must be a finite number > 0, got %r" % (lam,))
    if not (tol >= 0.0 and np.isfinite(tol)):
        raise ValueError("tol must be finite and not negative, got %r" % (tol,))
    return SvPoseGraphSpec(lam, tol)


def _pose_graph_edges(fixed, i, j, w, words, dev):
    """fixed, i, j, w and the incidence lists as the C entries take them -> (N, E, the six tensors).  words: pose_graph_words' pair (numpy
    or tensors), or None to make it here - which reads i and j back where they are tensors."""
    import torch
    from .stereo_vision import sv as _sv
    N = int(fixed.shape[0]) if hasattr(fixed, "shape") else len(fixed)
    E = int(i.shape[0]) if hasattr(i, "shape") else len(i)
    if not (1 <= N <= _sv.POSE_GRAPH_POSES_MAX and 0 <= E <= _sv.POSE_GRAPH_EDGES_MAX):
        raise ValueError("a pose graph holds 1 .. 2^20 poses and 0 .. 2^22 edges, got %d and %d" % (N, E))
    if words is None:
        as_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        i_np, j_np = as_np(i).astype(np.int64), as_np(j).astype(np.int64)
        if ((i_np < 0) | (i_np >= N) | (j_np < 0) | (j_np >= N) | (i_np == j_np)).any():
            raise ValueError("an edge names a pose outside 0 .. %d, or one pose twice" % (N - 1))
        words = _sv.pose_graph_words(N, i_np, j_np)
    fixed = _pose_graph_tensor(fixed, torch.uint8, (N,), dev, "fixed")
    i, j = _pose_graph_tensor(i, torch.int32, (E,), dev, "i"), _pose_graph_tensor(j, torch.int32, (E,), dev, "j")
    w = _pose_graph_tensor(w, torch.float64, (E, 2), dev, "w")
    row_start = _pose_graph_tensor(words[0], torch.int32, (N + 1,), dev, "row_start")
    inc = _pose_graph_tensor(words[1], torch.int32, (2 * E,), dev, "inc")
    return N, E, (fixed, i, j, w, row_start, inc)


def pose_graph_linearize(poses, fixed, i, j, Z, w, lam, words=None, out=None):
    """One linearisation of a pose graph - the definition of stereo_vision.sv.pose_graph_linearize on the GPU, bit for bit
    (sv_pose_graph_linearize_device: two kernels, doubles, no atomics).  poses a CUDA float64 tensor [N,12]; fixed bool or uint8 [N], i,
    j int32 [E], Z float64 [E,12], w float64 [E,2] - tensors on that device or numpy arrays, uploaded; words: pose_graph_words' pair, made
    here where None; out: the dict of an earlier call of the same shape to write into.  -> {"M" [E,12], "Wr" [E,6], "chi2" [E], "b"
    [N,6], "factor" [N,21]: float64 tensors, "words": the pair on the device}, enqueued on torch's current stream; nothing is read back
    where words is given.  The checks of the graph are stereo_vision.sv.pose_graph's: this entry only skips what points outside.  CPU
    tensors (or numpy arrays) run the numpy form and give numpy arrays."""
    import torch
    if not (isinstance(poses, torch.Tensor) and poses.is_cuda):
        from .stereo_vision.sv import pose_graph_linearize as on_host
        as_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t
        return on_host(as_np(poses), as_np(fixed), as_np(i), as_np(j), as_np(Z), as_np(w), lam, None if words is None else tuple(as_np(t) for t in words))
    dev = poses.device
    spec = _pose_graph_spec(lam, 0.0)
    N, E, (fixed, i, j, w, row_start, inc) = _pose_graph_edges(fixed, i, j, w, words, dev)
    poses = _pose_graph_tensor(poses, torch.float64, (N, 12), dev, "poses")
    Z = _pose_graph_tensor(Z, torch.float64, (E, 12), dev, "Z")
    res = _place_outputs(None if out is None else {k: v for k, v in out.items() if k != "words"},
                         (("M", torch.float64, (E, 12)), ("Wr", torch.float64, (E, 6)), ("chi2", torch.float64, (E,)), ("b", torch.float64, (N, 6)),
                          ("factor", torch.float64, (N, 21))), dev)
    with torch.cuda.device(dev):
        rc = pose_graph_lib().sv_pose_graph_linearize_device(poses.data_ptr(), fixed.data_ptr(), N, _ptr(i), _ptr(j), _ptr(Z), _ptr(w), E, row_start.data_ptr(), _ptr(inc),
                                                             ctypes.byref(spec), _ptr(res["M"]), _ptr(res["Wr"]), _ptr(res["chi2"]), res["b"].data_ptr(),
                                                             res["factor"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    _check(rc, "sv_pose_graph_linearize_device")
    res["words"] = (row_start, inc)
    return res


def pose_graph_solve(fixed, i, j, w, lin, lam, max_iters=1000, tol=1e-8, round=16, x=None, workspace=None):
    """Preconditioned conjugate gradients on a linearised pose graph - the definition of stereo_vision.sv.pose_graph_pcg on the GPU, bit
    for bit (sv_pose_graph_pcg_device: three kernels per iteration, no atomics).  lin: pose_graph_linearize's dict, CUDA tensors; fixed,
    i, j, w as given there.  x: a float64 tensor [N,6] to write into; workspace: a uint8 tensor of at least sv_pose_graph_workspace's
    bytes to reuse.  The C entry is called in rounds of `round` iterations (1 .. 1024; the last is cut to what max_iters leaves) and
    enqueues on torch's current stream without waiting; after each round the 16 bytes of iteration, done and rr are read back - the only
    wait - and the rounds stop once done is set, or after max_iters.  -> x, {"iteration", "done", "rr", "rr0"}, the state as
    pose_graph_pcg gives it.  CPU tensors (or numpy arrays) run the numpy form."""
    import torch
    from .stereo_vision import sv as _sv
    if not (isinstance(lin["b"], torch.Tensor) and lin["b"].is_cuda):
        as_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t
        return _sv.pose_graph_pcg(as_np(fixed), as_np(i), as_np(j), as_np(w), as_np(lin["M"]), as_np(lin["b"]), as_np(lin["factor"]), lam, max_iters, tol,
                                  None if lin.get("words") is None else tuple(as_np(t) for t in lin["words"]))
    dev = lin["b"].device
    spec = _pose_graph_spec(lam, tol)
    for v, lo, hi, what in ((max_iters, 0, 2 ** 30, "max_iters"), (round, 1, 1024, "round")):
        if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    N, E, (fixed, i, j, w, row_start, inc) = _pose_graph_edges(fixed, i, j, w, lin.get("words"), dev)
    M = _pose_graph_tensor(lin["M"], torch.float64, (E, 12), dev, "M")
    b = _pose_graph_tensor(lin["b"], torch.float64, (N, 6), dev, "b")
    F = _pose_graph_tensor(lin["factor"], torch.float64, (N, 21), dev, "factor")
    x = torch.empty((N, 6), dtype=torch.float64, device=dev) if x is None else _pose_graph_tensor(x, torch.float64, (N, 6), dev, "x")
    L = pose_graph_lib()
    nbytes = ctypes.c_size_t()
    _check(L.sv_pose_graph_workspace(N, E, ctypes.byref(nbytes)), "sv_pose_graph_workspace")
    if workspace is None:
        workspace = torch.empty(nbytes.value, dtype=torch.uint8, device=dev)
    elif not (isinstance(workspace, torch.Tensor) and workspace.device == dev and workspace.dtype == torch.uint8 and workspace.is_contiguous()
              and workspace.numel() >= nbytes.value):
        raise ValueError("workspace must be a contiguous uint8 tensor of at least %d bytes on %s" % (nbytes.value, dev))
    enqueued, first, state = 0, True, None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        while first or (enqueued < max_iters and not state[1]):
            n = min(int(round), int(max_iters) - enqueued)
            rc = L.sv_pose_graph_pcg_device(fixed.data_ptr(), N, _ptr(i), _ptr(j), _ptr(w), E, row_start.data_ptr(), _ptr(inc), _ptr(M), b.data_ptr(), F.data_ptr(),
                                            ctypes.byref(spec), enqueued, n, x.data_ptr(), workspace.data_ptr(), workspace.numel(), stream)
            _check(rc, "sv_pose_graph_pcg_device")
            state = workspace[:16].cpu().numpy().view(np.int32)  # 16 bytes: the wait of the round
            enqueued += n
            first = False
        words = workspace[:24].cpu().numpy()
    return x, {"iteration": int(words[:4].view(np.int32)[0]), "done": bool(words[4:8].view(np.int32)[0]), "rr": float(words[8:16].view(np.float64)[0]),
               "rr0": float(words[16:24].view(np.float64)[0])}


def pose_graph_optimize(graph, rounds=10, gate=None, eps=1e-9, lam=1e-6, max_iters=None, tol=1e-8, device=None, device_edges=None, checked=False, wrap_step=None):
    """stereo_vision.sv.pose_graph_optimize with every round's linearise and solve on the GPU: the same poses, costs, iterations and
    switched-off edges as the numpy form, bit for bit, since the device gives the same delta and chi2 and everything else is the same
    host code.  graph: stereo_vision.sv.pose_graph's dict; its arrays may be numpy arrays or tensors.  The GPU path is taken where
    `device` names a CUDA device or graph["poses"] is a CUDA tensor; the edges, the incidence lists and the fixed mask are uploaded once,
    poses and weights once per round, and delta [N,6] and chi2 [E] are read back once per round - the round's one wait besides the
    solver's 16 bytes per sixteen iterations.  device_edges: {"i", "j", "Z"} as tensors on the device that hold the graph's edges already
    (rig.PoseGraph's), used where they lie instead of an upload; checked=True: graph is stereo_vision.sv.pose_graph's own dict, all numpy,
    and is not checked again; wrap_step: a function that takes the round's step and returns the one to call - a hook for timing.
    max_iters None is max(1000, 20 N).  -> poses (numpy [N,12]), the stats dict."""
    import torch
    from .stereo_vision import sv as _sv
    as_np = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if device is None and isinstance(graph["poses"], torch.Tensor) and graph["poses"].is_cuda:
        device = graph["poses"].device
    if checked:
        host = graph
    else:
        host = {k: as_np(v) for k, v in graph.items()}
        host = _sv.pose_graph(host["poses"], [(host["i"], host["j"], host["Z"], host["w"], host["kind"])], host["fixed"].astype(bool))
    wrap = (lambda f: f) if wrap_step is None else wrap_step
    if device is None:
        return _sv.pose_graph_optimize(host, rounds, gate, eps, lam, max_iters, tol, step=wrap(_sv.pose_graph_step))
    dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    N, E = len(host["poses"]), len(host["i"])
    kept = {}

    def step(g, poses, w, lam, max_iters, tol, words):
        if not kept:
            on = device_edges or g
            _, _, t = _pose_graph_edges(g["fixed"], on["i"], on["j"], w, words, dev)
            kept["fixed"], kept["i"], kept["j"], kept["words"] = t[0], t[1], t[2], (t[4], t[5])
            kept["Z"] = _pose_graph_tensor(on["Z"], torch.float64, (E, 12), dev, "Z")
            kept["lin"], kept["x"] = None, None
        P, w = torch.from_numpy(np.ascontiguousarray(poses)).to(dev), torch.from_numpy(np.ascontiguousarray(w)).to(dev)
        kept["lin"] = pose_graph_linearize(P, kept["fixed"], kept["i"], kept["j"], kept["Z"], w, lam, kept["words"], kept["lin"])
        x, state = pose_graph_solve(kept["fixed"], kept["i"], kept["j"], w, kept["lin"], lam, max_iters, tol, x=kept["x"])
        kept["x"] = x
        return x.cpu().numpy(), kept["lin"]["chi2"].cpu().numpy(), state

    return _sv.pose_graph_optimize(host, rounds, gate, eps, lam, max_iters, tol, step=wrap(step))


def debug_place(one_key=0):
    """sv_debug_place: one_key = 1 lets a wavefront of the search take one key per pass instead of four - the same results, for timing
    only.  0 is the default.  Process-wide; a measurement hook."""
    _check(place_lib().sv_debug_place(int(one_key)), "sv_debug_place")


def host_support_filter(params, dcan, width, height, threads=0, lattice=False):
    """Product host stage: lattice filters + corner points (CPU by design; see csrc/host_stage.h).  threads > 0: the lattice shared between
    that many threads (what single-pair calls do); lattice=True: also return the filtered lattice."""
    d = np.ascontiguousarray(dcan, dtype=np.int16).copy()
    cap = d.size + 6
    out = np.empty((cap, 3), np.int32)
    if threads > 0:
        n = lib().sv_host_support_filter_threads(ctypes.byref(params), d.ctypes.data, width, height, out.ctypes.data, cap, threads)
    else:
        n = lib().sv_host_support_filter(ctypes.byref(params), d.ctypes.data, width, height, out.ctypes.data, cap)
    if n < 0:
        raise StereoError("support capacity")
    return (out[:n].copy(), d) if lattice else out[:n].copy()


def gpu_support_filter(params, lattices, width, height, stats=False, prime=None):
    """The same filters by the kernels of the GPU lattice filter (test hook, sv_gpu_support_filter): lattices int16 [n, Hc, Wc] (or one
    [Hc, Wc]), all filtered by one launch.  Returns (lists, counts): lists[i] the (k, 3) int32 support points of lattice i; with stats=True
    also int32 [n, 3] = uncertain points, refinement rounds run, points left to the sequential rest.  prime: as many lattices of the same
    size that go through the same workspace first.  The library refuses (StereoError) parameters the engine keeps on the host and lattices
    the support matching cannot have written."""
    share_hip_runtime_with_torch()
    lat = np.ascontiguousarray(lattices, dtype=np.int16)
    if lat.ndim == 2:
        lat = lat[None]
    if lat.ndim != 3 or lat.shape[0] < 1:
        raise ValueError("lattices must be int16 [n,Hc,Wc]")
    pr = None
    if prime is not None:
        pr = np.ascontiguousarray(prime, dtype=np.int16).reshape((-1,) + lat.shape[1:])
        if pr.shape != lat.shape:
            raise ValueError("prime must have the shape of lattices")
    step = params.candidate_stepsize + (params.candidate_stepsize % 2 if params.subsampling else 0)
    if step < 1 or lat.shape[1:] != ((height + step - 1) // step, (width + step - 1) // step):
        raise ValueError("a %d x %d image at step %d has another lattice than %s" % (width, height, step, lat.shape[1:]))
    n, cap = lat.shape[0], (lat.shape[1] - 1) * (lat.shape[2] - 1) + 6
    out, counts, st = np.zeros((n, cap, 3), np.int32), np.zeros(n, np.int32), np.zeros((n, 3), np.int32)
    L = lib()
    L.sv_gpu_support_filter.argtypes = [ctypes.POINTER(SvParams), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_void_p, ctypes.c_void_p]
    L.sv_gpu_support_filter.restype = ctypes.c_int
    rc = L.sv_gpu_support_filter(ctypes.byref(params), lat.ctypes.data, None if pr is None else pr.ctypes.data, n, int(width), int(height), out.ctypes.data, cap, counts.ctypes.data,
                                 st.ctypes.data if stats else None)
    if rc != 0:
        raise StereoError("sv_gpu_support_filter failed (%d): %s" % (rc, L.sv_last_error(None).decode()))
    lists = [out[i, :counts[i]].copy() for i in range(n)]
    return (lists, counts, st) if stats else (lists, counts)


def gpu_delaunay(xy, reps=1):
    """Triangulation with the divide-and-conquer phase on the GPU (test hook).  Returns (triangles (nt,3) int32, kernel ms)."""
    share_hip_runtime_with_torch()
    xy = np.ascontiguousarray(xy, dtype=np.int32)
    n = xy.shape[0]
    out = np.empty((2 * n + 8, 3), np.int32)
    ms = ctypes.c_double(0.0)
    L = lib()
    L.sv_gpu_delaunay.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
    nt = L.sv_gpu_delaunay(xy.ctypes.data, n, out.ctypes.data, 2 * n + 8, int(reps), ctypes.byref(ms))
    if nt < 0:
        raise StereoError("sv_gpu_delaunay failed (%d): %s" % (nt, L.sv_last_error(None).decode()))
    return out[:nt].copy(), ms.value


def host_kd_order(xy):
    """Test hook: ids of the vertices that survive the duplicate scan, in the order the triangulation's recursion consumes them
    (host: radix sort / the reference's quicksort when points coincide, duplicate scan, k-d order)."""
    xy = np.ascontiguousarray(xy, dtype=np.int32)
    out = np.empty(xy.shape[0], np.int32)
    L = lib()
    L.sv_host_kd_order.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    m = L.sv_host_kd_order(xy.ctypes.data, xy.shape[0], out.ctypes.data)
    if m < 0:
        raise StereoError("sv_host_kd_order failed (%d)" % m)
    return out[:m].copy()


def gpu_kd_order(xy, width, height, step, disp_max, disp=None):
    """Test hook: the same on the GPU (delaunay_gpu.hip: dg_prepare) for vertices on the support lattice of a width x height image;
    disp: the vertices' disparities (coincident vertices with equal disparity are interchangeable: the lowest id is kept).  None for
    a set the kernel leaves to the host (coincident points that are not interchangeable)."""
    share_hip_runtime_with_torch()
    xy = np.ascontiguousarray(xy, dtype=np.int32)
    out = np.empty(xy.shape[0], np.int32)
    dp = None
    if disp is not None:
        disp = np.ascontiguousarray(disp, dtype=np.int32)
        assert disp.shape[0] == xy.shape[0]
        dp = disp.ctypes.data
    L = lib()
    L.sv_gpu_kd_order.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    m = L.sv_gpu_kd_order(xy.ctypes.data, dp, xy.shape[0], int(width), int(height), int(step), int(disp_max), out.ctypes.data)
    if m == -1:
        return None
    if m < 0:
        raise StereoError("sv_gpu_kd_order failed (%d)" % m)
    return out[:m].copy()


def host_delaunay(xy, split=False, helper_delay_us=0, depth=1):
    """Product host stage: Delaunay triangulation of integer points (n,2) -> (nt,3) int32.  split: build the halves (depth 2:
    quarters) of the top-level cuts on other threads (what the engine does in latency mode)."""
    xy = np.ascontiguousarray(xy, dtype=np.int32)
    n = xy.shape[0]
    out = np.empty((2 * n + 8, 3), np.int32)
    if split:
        L = lib()
        L.sv_host_delaunay_par.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        nt = L.sv_host_delaunay_par(xy.ctypes.data, n, out.ctypes.data, 2 * n + 8, int(depth), int(helper_delay_us))
    else:
        nt = lib().sv_host_delaunay(xy.ctypes.data, n, out.ctypes.data, 2 * n + 8)
    if nt < 0:
        raise StereoError("triangle capacity")
    return out[:nt].copy()
