"""A calibrated stereo camera as a handle (sv_rig_* of include/stereo_vision_hip.h): camera frames in, the engine's input,
disparity, the driver's 8-bit map and point clouds out.

    rig = StereoRig(1242, 375, calibration=DEFAULT_CALIBRATION, rectify=False, scale=1.0)
    rig.Q, rig.XR, rig.XT                                            # numpy; XR / XT are None when the file has none
    gl, gr = rig.frontend(left, right, pixel_format="bgr")           # u8 [B,H,W]
    d1 = rig.disparity(left, right, pixel_format="bgr")              # f32 [B,H,W]
    d1, dmap, points = rig.point_clouds(left, right, pixel_format="bgr")
    grid = rig.top_view(left, right, (0, 40), (-20, 20), (-1.4, 1.0), 10, disparity="d1", transform=(CAMERA_TO_VEHICLE, None))
    pos, stat = rig.box_positions(left, right, boxes, n_boxes)       # f64 [B,M,3] metres, int32 [B,M,4]
    xyz, color, counts = rig.compact_clouds(left, right, lo=(0, -20, -1.4), hi=(40, 20, 1.0), transform=(CAMERA_TO_VEHICLE, None))
    clouds = split_clouds(xyz, counts, color)                        # per frame (f32 [n,3] metres, BGRA u8 [n,4]), in pixel order
    xyz, color, n, counts = rig.voxel_clouds(left, right, 0.1, (0, -20, -1.4), (40, 20, 1.0), transform=(CAMERA_TO_VEHICLE, None), capacity=65536)
    voxels = split_voxel_clouds(xyz, counts, color, n)               # per frame (centroids f32 [V,3], mean BGRA u8 [V,4], points per voxel)
    g = rig.ground(left, right)                                      # g.ground [B,4] = (vh, qb, S, n_valid), g.labels u8 [B,H,W], g.free_row [B,W],
                                                                     # g.pose[b] = (height m, pitch rad, slope), g.points f64 [B,W,3] metres
    o = rig.objects(left, right)                                     # no detector: o.boxes int32 [B,64,4] = (x, y, w, h), o.counts [B],
                                                                     # o.positions f64 [B,64,3] metres, o.stixels int32 [B,layers,W,4]
    occ = rig.occupancy(left, right, (0, 40), (-20, 20), (-1.4, 1.0), 10, transform=(CAMERA_TO_VEHICLE, None))
                                                                     # occ.state u8 [B,401,401] (0 unknown, 1 free, 2 occupied), occ.cells
                                                                     # int32 [B,401,401,4] = (n_ground, n_obstacle, h_lo, h_hi), occ.n_rays
    world = rig.occupancy_map((-50, 150), (-100, 100), 10)           # a world-fixed log-odds map of 2000 x 2000 uniform cells
    world.update(occ, occupancy_pose(x, y, yaw))                     # the frames' states fused along the poses of the odometry, in order
    world.recenter(x[-1], y[-1])                                     # scrolled by whole cells: the vehicle in the middle cell
    world.state()                                                    # u8 [2000,2000] (0 unknown, 1 free, 2 occupied) by thresholds on log-odds
    xyyaw, m = world.localize(occ, guess, (0.5, 0.5, 0.04), (7, 7, 5))  # per frame the best pose of a 245-pose window around the odometry's
                                                                     # guess [B,3]; m.sums / m.counts / m.best / m.best_score on the device
    model = rig.voxel_map((-50, -100, -2), (150, 100, 4), 0.1, 1 << 21)  # a world-fixed voxel map: one coloured 3-D model of a drive
    model.update(xyz, color, n, counts, voxel_map_pose(x, y, yaw))   # voxel_clouds' (or compact_clouds') rows fused along the same odometry
    xyzyaw, m = model.localize(xyz, n, counts, guess, (0.5, 0.5, 0.2, 0.04), (5, 5, 3, 5))  # per frame the best pose of a 375-pose window
                                                                     # around the guess [B,4], before the frame is inserted there
    model.write_ply("drive.ply", min_rows=2)                         # the voxels that at least two rows fell into, ordered by cell

Frames are [B,Hs,Ws,C] (C = 4, 3, 3 for "bgra", "bgr", "rgb") or [B,Hs,Ws] for "gray"; one frame without B is accepted.
Frames of another size than the rig's are resized to it.  CUDA tensors are processed on torch's current stream and CUDA
tensors come back; numpy arrays go up through page-locked staging and numpy arrays come back.  Rows may be padded (a slice of
a wider tensor); frames must lie back to back.
"""
import ctypes

import numpy as np

from .engine import disparity_warp, flow_egomotion, flow_match, object_links, place_descriptor, place_match, pose_graph_optimize
from .engine import (SvParams, StereoEngine, StereoError, box_positions_from_disparity, box_spec, cloud_spec, compact_cloud_from_disparity,
                     ground_from_disparity, ground_spec, lib, occupancy_from_disparity, occupancy_fuse, occupancy_match, occupancy_clearance, clearance_paths, cost_cells, cost_routes, frontier_cells, frontier_clusters, occupancy_cost_to_goal, occupancy_view, occupancy_spec, pinned_array, reproject, split_clouds, stixel_spec, stixels_from_disparity,
                     top_view_from_disparity, top_view_spec, split_voxel_clouds, voxel_cloud_from_disparity, voxel_map_align, voxel_map_carry, voxel_map_clear, voxel_map_insert, voxel_map_match, voxel_map_new, voxel_map_repose,
                     voxel_map_rows, voxel_map_stats, voxel_spec)
from .stereo_vision.sv import CAMERA_TO_VEHICLE, DEFAULT_CALIBRATION  # noqa: F401 (CAMERA_TO_VEHICLE: re-exported for top_view)
from .stereo_vision.sv import free_space_points, ground_pose
from .stereo_vision import sv as _sv

PIXEL_FORMATS = {"bgra": 0, "bgr": 1, "rgb": 2, "gray": 3}
_CHANNELS = {"bgra": 4, "bgr": 3, "rgb": 3, "gray": 1}
SV_ERR_ARG = -1


class SvRigConfig(ctypes.Structure):
    """sv_rig_config of include/stereo_vision_hip.h."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("device", ctypes.c_int32), ("rectify", ctypes.c_int32),
                ("scale", ctypes.c_float), ("reserved", ctypes.c_int32 * 3)]


_bound = False


def rig_lib():
    """The library with the sv_rig_* signatures declared."""
    global _bound
    L = lib()
    if not _bound:
        vp = ctypes.c_void_p
        L.sv_rig_create.argtypes = [ctypes.c_char_p, ctypes.POINTER(SvRigConfig), ctypes.POINTER(vp)]
        L.sv_rig_create.restype = ctypes.c_int
        L.sv_rig_destroy.argtypes = [vp]
        L.sv_rig_destroy.restype = ctypes.c_int
        L.sv_rig_last_error.argtypes = [vp]
        L.sv_rig_last_error.restype = ctypes.c_char_p
        L.sv_rig_matrices.argtypes = [vp, vp, vp, vp]
        L.sv_rig_matrices.restype = ctypes.c_int
        L.sv_rig_maps.argtypes = [vp, vp]
        L.sv_rig_maps.restype = ctypes.c_int
        L.sv_rig_frontend_device.argtypes = [vp, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
        L.sv_rig_frontend_device.restype = ctypes.c_int
        _bound = True
    return L


class StereoRig:
    def __init__(self, width, height, calibration=DEFAULT_CALIBRATION, rectify=False, scale=1.0, params=None, device=0, **engine_kwargs):
        """params: the engine's SvParams (default SvParams.driver(255), what generatePointCloud runs); engine_kwargs go to StereoEngine,
        which is created by the first disparity() / point_clouds() call (a rig used for its front end only holds no engine)."""
        L = rig_lib()
        self.width, self.height, self.device = int(width), int(height), int(device)
        self.rectify = bool(rectify)
        self.params = params if params is not None else SvParams.driver(255)
        self._engine_kwargs = engine_kwargs
        self._engine = None
        self._stage = {}
        cfg = SvRigConfig(self.width, self.height, self.device, int(self.rectify), float(scale))
        h = ctypes.c_void_p()
        rc = L.sv_rig_create(str(calibration).encode(), ctypes.byref(cfg), ctypes.byref(h))
        if rc != 0:
            msg = "sv_rig_create failed (%d): %s" % (rc, L.sv_rig_last_error(None).decode())
            raise ValueError(msg) if rc == SV_ERR_ARG else StereoError(msg)
        self._h = h
        Q, XR, XT = np.zeros(16), np.zeros(9), np.zeros(3)
        has = L.sv_rig_matrices(self._h, Q.ctypes.data, XR.ctypes.data, XT.ctypes.data)
        self.Q = Q.reshape(4, 4)
        self.XR = XR.reshape(3, 3) if has & 1 else None
        self.XT = XT if has & 2 else None

    def close(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        if getattr(self, "_h", None):
            rig_lib().sv_rig_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def maps(self):
        """[4,H,W] float32 lmapx, lmapy, rmapx, rmapy (initUndistortRectifyMap), or None when rectification is off."""
        if not self.rectify:
            return None
        m = np.zeros((4, self.height, self.width), np.float32)
        self._check(rig_lib().sv_rig_maps(self._h, m.ctypes.data))
        return m

    @property
    def engine(self):
        if self._engine is None:
            self._engine = StereoEngine(self.width, self.height, self.params, device=self.device, **self._engine_kwargs)
        return self._engine

    def _check(self, rc):
        if rc != 0:
            msg = "libstereo_vision_hip error %d: %s" % (rc, rig_lib().sv_rig_last_error(self._h).decode())
            raise ValueError(msg) if rc == SV_ERR_ARG else StereoError(msg)

    # ---- inputs
    def _frames(self, x, fmt, side):
        """-> (CUDA uint8 tensor [B,Hs,Ws(,C)] with unit pixel strides, row pitch in bytes, came_from_numpy)."""
        import torch
        C = _CHANNELS[fmt]
        nd = 3 if C == 1 else 4
        from_numpy = isinstance(x, np.ndarray)
        if from_numpy:
            x = np.asarray(x)
            if x.dtype != np.uint8:
                raise ValueError("frames must be uint8")
            if x.ndim == nd - 1:
                x = x[None]
            if x.ndim != nd:
                raise ValueError("expected %s frames [B,H,W%s], got shape %s" % (fmt, "" if C == 1 else ",%d" % C, x.shape))
            buf = self._stage.get(side)
            if buf is None or buf.size < x.size:
                buf = pinned_array((x.size,), np.uint8)
                self._stage[side] = buf
            stage = buf[:x.size].reshape(x.shape)
            np.copyto(stage, x)
            x = torch.from_numpy(stage).to(torch.device("cuda", self.device), non_blocking=True)
        elif not (isinstance(x, torch.Tensor) and x.is_cuda):
            raise ValueError("frames must be numpy arrays or CUDA tensors")
        if x.dtype != torch.uint8:
            raise ValueError("frames must be uint8")
        if x.device != torch.device("cuda", self.device):
            raise ValueError("frames must be on cuda:%d (the rig's device)" % self.device)
        if x.dim() == nd - 1:
            x = x.unsqueeze(0)
        if x.dim() != nd or (C > 1 and x.shape[3] != C):
            raise ValueError("expected %s frames [B,H,W%s], got shape %s" % (fmt, "" if C == 1 else ",%d" % C, tuple(x.shape)))
        B, Hs, Ws = x.shape[:3]
        pix = (x.stride(3) == 1 and x.stride(2) == C) if C > 1 else x.stride(2) == 1
        if not pix or x.stride(1) < Ws * C or (B > 1 and x.stride(0) != Hs * x.stride(1)):
            x = x.contiguous()
        return x, x.stride(1), from_numpy

    def _run_frontend(self, left, right, pixel_format, colors):
        import torch
        fmt = str(pixel_format).lower()
        if fmt not in PIXEL_FORMATS:
            raise ValueError("pixel_format must be one of %s" % sorted(PIXEL_FORMATS))
        l, pitch, from_numpy = self._frames(left, fmt, 0)
        r, rpitch, _ = self._frames(right, fmt, 1)
        if tuple(l.shape) != tuple(r.shape) or pitch != rpitch:
            raise ValueError("left and right frames differ in shape or row pitch: %s / %s" % (tuple(l.shape), tuple(r.shape)))
        B, Hs, Ws = l.shape[:3]
        dev = l.device
        gl = torch.empty((B, self.height, self.width), dtype=torch.uint8, device=dev)
        gr = torch.empty_like(gl)
        col = torch.empty((B, self.height, self.width, 4), dtype=torch.uint8, device=dev) if colors else None
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            self._check(rig_lib().sv_rig_frontend_device(self._h, l.data_ptr(), r.data_ptr(), B, Ws, Hs, pitch, PIXEL_FORMATS[fmt], gl.data_ptr(),
                                                         gr.data_ptr(), col.data_ptr() if col is not None else None, st))
        return gl, gr, col, from_numpy

    def _transform(self, transform):
        """-> (XR, XT) of a transform argument: None, "rig" (the calibration file's; ValueError if it has none) or (XR, XT)."""
        if transform is None:
            return None, None
        if isinstance(transform, str) and transform == "rig":
            if self.XR is None and self.XT is None:
                raise ValueError("transform=\"rig\": the calibration file has no XR / XT")
            return self.XR, self.XT
        if isinstance(transform, (tuple, list)) and len(transform) == 2:
            return transform[0], transform[1]
        raise ValueError("transform must be None, \"rig\" or (XR, XT)")

    # ---- public
    def frontend(self, left, right, pixel_format="bgr", colors=False):
        """-> (gray_left, gray_right) u8 [B,H,W] (+ the left colours BGRA [B,H,W,4] with colors=True), enqueued on torch's current stream."""
        gl, gr, col, from_numpy = self._run_frontend(left, right, pixel_format, colors)
        out = (gl, gr) + ((col,) if colors else ())
        return tuple(t.cpu().numpy() for t in out) if from_numpy else out

    def disparity(self, left, right, pixel_format="bgr"):
        """Left disparity maps f32 [B,H,W] of the engine (params of the rig) on the front end's images."""
        gl, gr, _, from_numpy = self._run_frontend(left, right, pixel_format, False)
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        return d1.cpu().numpy() if from_numpy else d1

    def point_clouds(self, left, right, pixel_format="bgr", colors=False):
        """-> (d1 f32 [B,H,W], dmap u8 [B,H,W] = saturate(round(4 d)), points f64 [B,H,W,3] = Q [x y dmap 1] / w[, colours BGRA [B,H,W,4]]):
        the reference driver's per-frame outputs (stereo_vision.cpp:316, 233-256), for a batch."""
        if self.params.subsampling:
            raise ValueError("point_clouds does not support half-resolution maps (params.subsampling)")
        gl, gr, col, from_numpy = self._run_frontend(left, right, pixel_format, colors)
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        dmap, pts = reproject(d1, self.Q)
        out = (d1, dmap, pts) + ((col,) if colors else ())
        return tuple(t.cpu().numpy() for t in out) if from_numpy else out

    def top_view(self, left, right, x_range, y_range, z_range, scale, pixel_format="bgr", mode="reference", disparity="dmap", transform=None):
        """Bird's-eye views [B,rows,cols] of B pairs (uint8 for mode "reference", int32 for "count"; the grid of
        stereo_vision.sv.points_2_top_view): front end, engine, then the fused disparity -> grid kernel - no point cloud is written.
        disparity "dmap": the points of point_clouds (the driver's convention, a quarter of metric depth); "d1": the float disparity
        reprojected, in metres, pixels with d <= 0 skipped.  transform: None, "rig" (the calibration file's XR / XT; ValueError if it
        has none) or (XR, XT) - point = XR (X, Y, Z) + XT, either may be None.  The helper's axes are (forward, left, up); the camera's
        are (right, down, forward), so a camera-fixed top view takes

            XR = [[0, 0, 1], [-1, 0, 0], [0, -1, 0]], XT = 0       (rig.CAMERA_TO_VEHICLE)

        e.g. rig.top_view(l, r, (0, 40), (-20, 20), (-1.4, 1.0), 10, disparity="d1", transform=(CAMERA_TO_VEHICLE, None))."""
        if self.params.subsampling:
            raise ValueError("top_view does not support half-resolution maps (params.subsampling)")
        top_view_spec(x_range, y_range, z_range, scale, mode, disparity)  # argument errors before any work
        XR, XT = self._transform(transform)
        gl, gr, _, from_numpy = self._run_frontend(left, right, pixel_format, False)
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        grid = top_view_from_disparity(d1, self.Q, x_range, y_range, z_range, scale, XR=XR, XT=XT, disparity=disparity, mode=mode)
        return grid.cpu().numpy() if from_numpy else grid

    def box_positions(self, left, right, boxes, n_boxes=None, pixel_format="bgr", select="near", disparity="d1", band=4, transform=None):
        """3-D position of each detected object of B pairs: (pos float64 [B,M,3], stat int32 [B,M,4] = (n_pixels, n_valid, q_med,
        n_selected)) for boxes int32 [B,M,4] = (x, y, w, h) in pixels of the rig's maps ([M,4] for one frame; n_boxes [B] = boxes in
        use per pair, rows beyond come back NaN / -1) - front end, engine, then the fused disparity -> positions kernel: no point
        cloud is written.  The defaults give metres from the float disparity ("d1"), over the valid pixels within `band` quarter
        pixels of the box's median disparity ("near": background inside the box is left out); select "valid" / "all" and disparity
        "dmap" (the driver's cloud, a quarter of metric depth; with "all" the reference's mean) as engine.box_positions_from_disparity.
        transform as in top_view: None (camera axes), "rig" or (XR, XT).  The boxes come from your own detector."""
        if self.params.subsampling:
            raise ValueError("box_positions does not support half-resolution maps (params.subsampling)")
        box_spec(select, disparity, band)  # argument errors before any work
        XR, XT = self._transform(transform)
        gl, gr, _, from_numpy = self._run_frontend(left, right, pixel_format, False)
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        pos, stat = box_positions_from_disparity(d1, self.Q, boxes, n_boxes, XR=XR, XT=XT, select=select, disparity=disparity, band=band)
        return (pos.cpu().numpy(), stat.cpu().numpy()) if from_numpy else (pos, stat)

    def compact_clouds(self, left, right, pixel_format="bgr", lo=None, hi=None, step=1, disparity="d1", dtype="f32", transform=None, capacity=None,
                       colors=True):
        """Coloured point clouds of B pairs as lists of points - what a viewer, a PLY file (stereo_vision.sv.write_ply) or a voxel grid
        takes: front end (with colours), engine, then the fused disparity -> compact cloud kernels; no dense cloud is written.  Per
        frame the pixels of every step-th column and row that carry a disparity and whose point lies strictly inside lo < P < hi (None =
        open; inf / NaN never pass), in pixel order.  disparity "d1": metres from the float disparity; "dmap": the driver's cloud, a
        quarter of metric depth.  transform as in top_view: None (camera axes), "rig" or (XR, XT); the crop applies after it.
        CUDA input: (xyz [B,capacity,3] float32 or float64 ("f64"), color BGRA uint8 [B,capacity,4] or None (colors=False), counts int32
        [B]) as engine.compact_cloud_from_disparity - rows at and beyond counts[b] are undefined, counts is not capped by capacity
        (None = the visited pixels: no overflow), nothing is waited for; engine.split_clouds cuts them.  numpy input: a list of
        per-frame (xyz [n,3], color [n,4] or None) numpy arrays."""
        if self.params.subsampling:
            raise ValueError("compact_clouds does not support half-resolution maps (params.subsampling)")
        cloud_spec(lo, hi, step, disparity, dtype)  # argument errors before any work
        XR, XT = self._transform(transform)
        gl, gr, col, from_numpy = self._run_frontend(left, right, pixel_format, bool(colors))
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        xyz, color, _, counts = compact_cloud_from_disparity(d1, self.Q, colors=col, XR=XR, XT=XT, lo=lo, hi=hi, step=step, disparity=disparity,
                                                             dtype=dtype, capacity=capacity)
        if not from_numpy:
            return xyz, color, counts
        return [(p.cpu().numpy(), None if c is None else c.cpu().numpy()) for p, c in split_clouds(xyz, counts, color)]

    def voxel_clouds(self, left, right, size, lo, hi, pixel_format="bgr", step=1, disparity="d1", dtype="f32", transform=None, capacity=None,
                     colors=True):
        """Voxel-grid downsampled coloured clouds of B pairs - what registration, a map or a planner takes instead of compact_clouds'
        lists: front end (with colours), engine, then the fused disparity -> voxel cloud kernels; neither a dense cloud nor the list
        of points is written.  One row per occupied cubic cell of edge `size` (metres with disparity "d1") of the finite crop
        lo < P < hi: the centroid, the mean colour and the number of points, in the order a scan of the image meets the cells.  step,
        disparity, dtype, transform as in compact_clouds; the crop applies after the transform.
        CUDA input: (xyz [B,capacity,3] float32 or float64 ("f64"), color BGRA uint8 [B,capacity,4] or None (colors=False), n int32
        [B,capacity], counts int32 [B]) as engine.voxel_cloud_from_disparity - counts[b] = -1 for a frame with more voxels than
        capacity (None = the visited pixels: no overflow, but a large workspace per pair - pass one for batches), rows at and beyond
        counts[b] are undefined, nothing is waited for; engine.split_voxel_clouds cuts them.  numpy input: a list of per-frame
        (xyz [V,3], color [V,4] or None, n [V]) numpy arrays."""
        if self.params.subsampling:
            raise ValueError("voxel_clouds does not support half-resolution maps (params.subsampling)")
        voxel_spec(size, lo, hi, step, disparity, dtype, capacity)  # argument errors before any work
        XR, XT = self._transform(transform)
        gl, gr, col, from_numpy = self._run_frontend(left, right, pixel_format, bool(colors))
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        xyz, color, _, n, _, counts = voxel_cloud_from_disparity(d1, self.Q, size, lo, hi, colors=col, XR=XR, XT=XT, step=step, disparity=disparity,
                                                                 dtype=dtype, capacity=capacity)
        if not from_numpy:
            return xyz, color, n, counts
        return [(p.cpu().numpy(), None if c is None else c.cpu().numpy(), k.cpu().numpy()) for p, c, k in split_voxel_clouds(xyz, counts, color, n)]

    def _flow_inputs(self, left, right, pixel_format):
        """Front end and engine once for a batch of consecutive pairs -> (gray left [B,H,W], d1 [B,H,W], the camera, came_from_numpy)."""
        if self.params.subsampling:
            raise ValueError("flow and odometry do not support half-resolution maps (params.subsampling)")
        gl, gr, _, from_numpy = self._run_frontend(left, right, pixel_format, False)
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        return gl, d1, self.render_camera(1.0), from_numpy

    def flow(self, left, right, pixel_format="bgr", guess=None, step=8, r=4, wx=8, wy=8, ratio=230, max_cost=225 * 255, capacity=8192):
        """The temporal matches of a batch of B consecutive pairs (include/stereo_vision_hip.h (Z1), stereo_vision.sv.flow_match): front
        end and engine once for the batch, then the lattice points of frame k - 1 that carry a disparity looked for in frame k, for k = 1
        .. B - 1, in one call.  guess: float64 [B-1,12], the expected motions, previous camera to current camera, or None - the identity.
        CUDA input: engine.FlowResult with matches int32 [B-1,capacity,6] = (u0, v0, d0q, u1, v1, d1q), cost int32 [B-1,capacity,2] and
        counts int32 [B-1] (-1: more matches than capacity); nothing is waited for.  numpy input: a dict of these as numpy arrays."""
        gl, d1, camera, from_numpy = self._flow_inputs(left, right, pixel_format)
        if gl.shape[0] < 2:
            raise ValueError("flow needs at least two consecutive pairs, got %d" % gl.shape[0])
        res = flow_match(gl[:-1], gl[1:], d1[:-1], d1[1:], camera, guess, step, r, wx, wy, ratio, max_cost, capacity)
        return {k: getattr(res, k).cpu().numpy() for k in ("matches", "cost", "counts")} if from_numpy else res

    def _odometry_pairs(self, gl, d1, camera, guess, spec):
        """stereo_vision.sv.flow_odometry over the B - 1 pairs of a batch whose front end and engine have run, with the device's calls."""
        s = _sv.flow_odometry_spec(**spec)
        words = {k: s[k] for k in ("step", "r", "ratio", "max_cost", "capacity")}

        def match_of(lo, hi, g, wx, wy):
            return flow_match(gl[lo:hi], gl[lo + 1:hi + 1], d1[lo:hi], d1[lo + 1:hi + 1], camera, g, wx=wx, wy=wy, **words)

        def ego_of(got, at):
            e = flow_egomotion(got.matches, got.counts, camera, at, s["gates"], s["dgate"], s["iterations"], s["eps"], s["min_inliers"])
            return {k: getattr(e, k) for k in ("poses", "ok", "rounds", "inliers")}

        return _sv.flow_odometry(match_of, ego_of, int(gl.shape[0]) - 1, guess, **spec)

    def odometry(self, left, right, pixel_format="bgr", start=None, transform=None, guess="velocity", **spec):
        """Stereo visual odometry of a batch of B consecutive pairs (include/stereo_vision_hip.h (Z), stereo_vision.sv.flow_odometry): front
        end and engine once for the batch; frame k matched against frame k - 1 and the camera's motion between them fitted by a gated
        Gauss-Newton loop whose sums come from the device (B x 32 words read back per round); the motions chained into poses.
        guess "velocity": the frames one after the other, each under the motion before it, the first over the cold-start window
        spec["cold"] (or under spec["first"], a motion [12]); "identity"; or the caller's motions [B-1,12].  start: the pose of frame 0
        ([12]; None: the identity); transform as in top_view - None, "rig" or (XR, XT), camera to frame: with (CAMERA_TO_VEHICLE, None) the
        poses are what VoxelMap.update, .align and --poses take.  spec: the words of stereo_vision.sv.FLOW_ODOMETRY.
        -> {"poses": float64 [B,12], frame to world; "rel": float64 [B-1,12], previous camera to current camera; "ok": bool [B-1];
        "inliers": int64 [B-1]; "matches": the matches of the B - 1 pairs - matches, cost and counts as flow() returns them, tensors for
        CUDA input and numpy arrays for numpy input}.  A pair whose fit was not ok repeats the motion before it in the chain."""
        import torch
        s = _sv.flow_odometry_spec(**spec)
        XR, XT = self._transform(transform)
        gl, d1, camera, from_numpy = self._flow_inputs(left, right, pixel_format)
        got = self._odometry_pairs(gl, d1, camera, guess, spec)

        calls = got["calls"]
        if calls:
            m = {k: torch.cat([getattr(c, k) for c in calls]) for k in ("matches", "cost", "counts")}
        else:
            dev = gl.device
            m = {"matches": torch.empty((0, s["capacity"], 6), dtype=torch.int32, device=dev), "cost": torch.empty((0, s["capacity"], 2), dtype=torch.int32, device=dev),
                 "counts": torch.empty((0,), dtype=torch.int32, device=dev)}
        if from_numpy:
            m = {k: v.cpu().numpy() for k, v in m.items()}
        return {"poses": _sv.flow_chain(got["rel"], start, XR, XT, got["ok"]), "rel": got["rel"], "ok": got["ok"], "inliers": got["inliers"], "matches": m}

    def temporal(self, left, right, pixel_format="bgr", poses=None, mode="fill", **words):
        """The disparity maps of a batch of B consecutive pairs made consistent with the frame before (include/stereo_vision_hip.h (AA),
        stereo_vision.sv.disparity_warp): front end and engine once for the batch, then the map of every frame k - 1 warped into frame k
        under the motion between them and compared with what frame k measured, for k = 1 .. B - 1, in one call.  poses: float64
        [B-1,12], previous camera to current camera - a row with a word that is not finite: a pair without a motion, not ok -, or None -
        odometry() with its defaults over the same maps.  mode "fill", "confirm"
        or "reject"; words: e_max, tol_q, rel_q.  -> {"d1": float32 [B,H,W], the maps with frames 1 .. B - 1 replaced by out; "label"
        uint8, "expected" and "source" int32 [B-1,H,W]; "counts" int32 [B-1,8]; "rel" float64 [B-1,12]; "ok" bool [B-1]} - tensors for
        CUDA input (rel and ok numpy), numpy arrays for numpy input.  A pair whose odometry fit was not ok keeps its measured map, and
        its labels are those of an empty frame before it: 0 and 1."""
        _sv.warp_words(mode=mode, **words)
        gl, d1, camera, from_numpy = self._flow_inputs(left, right, pixel_format)
        B = int(gl.shape[0])
        if B < 2:
            raise ValueError("temporal needs at least two consecutive pairs, got %d" % B)
        if poses is None:
            got = self._odometry_pairs(gl, d1, camera, "velocity", {})
            rel, ok = got["rel"], got["ok"]
        else:
            rel = np.array(poses, np.float64)
            if rel.shape != (B - 1, 12):
                raise ValueError("poses must be None or motions [%d,12], got shape %s" % (B - 1, rel.shape))
            ok = np.isfinite(rel).all(1)  # a motion with a word that is not finite stands for a pair without one
        used = rel.copy()
        used[~ok] = np.nan  # no source is kept under such a motion
        res = disparity_warp(d1[:-1], d1[1:], camera, used, mode=mode, **words)
        new = d1.clone()
        new[1:] = res.out
        for k in np.flatnonzero(~ok):
            new[k + 1] = d1[k + 1]
        out = {"d1": new, "label": res.label, "expected": res.expected, "source": res.source, "counts": res.counts}
        if from_numpy:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        out["rel"], out["ok"] = rel, ok
        return out

    def track(self, left, right, pixel_format="bgr", boxes=None, n_boxes=None, transform=None, guess="velocity", band_q=48, min_votes=3, share=128, gate_m=256,
              objects=None, **spec):
        """The objects of a batch of B consecutive pairs carried from frame to frame (include/stereo_vision_hip.h (AB),
        stereo_vision.sv.object_links): front end and engine once for the batch; odometry()'s matches and motions (guess and spec: its
        words); per frame the boxes of objects() (`objects`: a dict of its spec words, or None) or the caller's - boxes int32 [B,M,4] = (x,
        y, w, h), n_boxes int32 [B] or None - with box_positions(select="near") for their positions and reference disparities; then
        engine.object_links for the B - 1 consecutive pairs in one call, twice for gate_m > 0: a round without a gate and one gated, in
        1/1024 m, about the first round's mean motion, whose B x M x 16 words are read back.  At most 64 boxes per frame take part: the
        first 64, and "left_out" [B] says how many did not.  band_q, min_votes, share: object_links' words.  transform as in top_view, for
        the positions only.
        -> {"boxes" int32 [B,M,4], "n" int32 [B], "positions" float64 [B,M,3], "stat" int32 [B,M,4], "votes" int32 [B-1,M,M+1], "link" int32
        [B-1,M,4], "sums" int64 [B-1,M,16]: tensors for CUDA input, numpy arrays for numpy input; and on the host "left_out" int64 [B], "centre"
        int32 [B-1,M,3] or None, "motion" float64 [B-1,M,3] - per box of frame k - 1 its own motion to frame k in metres per frame, in the
        current camera's axes, NaN without a link or a match -, "count" int64 [B-1,M] - the matches behind it -, "rel" float64 [B-1,12],
        "ok" bool [B-1], "matches": odometry()'s}.  A pair whose odometry fit was not ok gets links from the votes but NaN motions."""
        import torch
        _sv.track_words(0, self.width, self.height, band_q, min_votes, share, gate_m)  # argument errors before any work
        _sv.flow_odometry_spec(**spec)
        XR, XT = self._transform(transform)
        gl, d1, camera, from_numpy = self._flow_inputs(left, right, pixel_format)
        B, dev = int(gl.shape[0]), gl.device
        if B < 2:
            raise ValueError("track needs at least two consecutive pairs, got %d" % B)
        if boxes is None:
            words = dict(objects or {})
            if words.get("min_support") is None:
                words["min_support"] = self.width
            stixel_words = {k: words.pop(k) for k in ("q_min", "sim", "max_gap", "min_rows", "max_layers", "col_step", "sim_cols", "min_cols") if k in words}
            g = ground_from_disparity(d1, self.params.disp_max, want_vdisp=False, want_free=False, **words)
            st = stixels_from_disparity(d1, g.labels, self.params.disp_max, capacity=_sv.TRACK_BOXES_MAX, want_stixels=False, **stixel_words)
            bx, found = st.boxes, st.counts
        else:
            bx = boxes if isinstance(boxes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(boxes, np.int32))
            if bx.dtype != torch.int32 or bx.dim() != 3 or tuple(bx.shape[::2]) != (B, 4):
                raise ValueError("boxes must be int32 [%d,M,4], got %s %s" % (B, bx.dtype, tuple(bx.shape)))
            bx = bx.to(dev)
            found = torch.full((B,), int(bx.shape[1]), dtype=torch.int32, device=dev) if n_boxes is None else \
                (n_boxes if isinstance(n_boxes, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(n_boxes, np.int32))).to(dev)
            if found.dtype != torch.int32 or tuple(found.shape) != (B,):
                raise ValueError("n_boxes must be None or int32 [%d]" % B)
            found = found.clamp(0, int(bx.shape[1]))
        bx = bx[:, :_sv.TRACK_BOXES_MAX].contiguous()
        M = int(bx.shape[1])
        n = found.clamp(0, M).to(torch.int32)
        left_out = (found.to(torch.int64) - M).clamp(min=0).cpu().numpy()
        if M:
            pos, stat = box_positions_from_disparity(d1, self.Q, bx, n, XR=XR, XT=XT, select="near", disparity="d1")
        else:
            pos, stat = torch.empty((B, 0, 3), dtype=torch.float64, device=dev), torch.empty((B, 0, 4), dtype=torch.int32, device=dev)
        q = stat[:, :, 2].contiguous()

        got = self._odometry_pairs(gl, d1, camera, guess, spec)
        rel, ok = got["rel"], got["ok"]
        m = {k: torch.cat([getattr(c, k) for c in got["calls"]]) for k in ("matches", "cost", "counts")}
        used = rel.copy()
        used[~ok] = np.nan  # no match is inside under such a motion: no sums, NaN motions
        res = _sv.object_links_rounds(lambda gate, centre: object_links(m["matches"], m["counts"], used, bx[:-1], n[:-1], q[:-1], bx[1:], n[1:], q[1:], camera, self.width,
                                                                        self.height, band_q, min_votes, share, gate, centre), gate_m)
        sums, link = res["sums"].cpu().numpy(), res["link"].cpu().numpy()
        mo = _sv.object_motion(sums, link)
        out = {"boxes": bx, "n": n, "positions": pos, "stat": stat, "votes": res["votes"], "link": res["link"], "sums": res["sums"]}
        if from_numpy:
            out = {k: v.cpu().numpy() for k, v in out.items()}
            m = {k: v.cpu().numpy() for k, v in m.items()}
        out.update(left_out=left_out, centre=res["centre"], motion=mo["motion"], count=mo["n"], rel=rel, ok=ok, matches=m)
        return out

    def ground(self, left, right, pixel_format="bgr", transform=None, **spec):
        """Where the ground is, what stands on it and how far one can go in each image column, for B pairs: front end, engine, then
        engine.ground_from_disparity on the float disparity (n_bins from the rig's disp_max; spec: vh_lo, vh_hi, vh_step, qb_step, tol,
        g_tol, min_run, min_support, want_vdisp, want_labels as there).  -> engine.GroundResult, with two host-side additions computed
        from the few words per pair and the one row per pair that are read back (this call waits for them): pose[b] = (height_m,
        pitch_rad, slope_px_per_row) of the camera over the fitted ground (stereo_vision.sv.ground_pose; None for a pair without
        ground) and points float64 numpy [B,W,3] = the 3-D point of each column's obstacle base in metres (free_space_points; NaN for a
        column without one), transform as in top_view: None (camera axes), "rig" or (XR, XT).  CUDA input: device tensors; numpy
        input: numpy arrays."""
        if self.params.subsampling:
            raise ValueError("ground does not support half-resolution maps (params.subsampling)")
        if "want_free" in spec or "disp_max" in spec or "n_bins" in spec:
            raise ValueError("ground: want_free, disp_max and n_bins are not options of the rig (the free space is always computed, the bins follow the rig's disp_max)")
        checked = {k: v for k, v in spec.items() if k not in ("want_vdisp", "want_labels")}
        if checked.get("min_support") is None:
            checked["min_support"] = self.width
        ground_spec(self.height, self.params.disp_max, **checked)  # argument errors before any work
        XR, XT = self._transform(transform)
        gl, gr, _, from_numpy = self._run_frontend(left, right, pixel_format, False)
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        res = ground_from_disparity(d1, self.params.disp_max, **spec)
        rec, row, dsp = res.ground.cpu().numpy(), res.free_row.cpu().numpy(), res.free_disp.cpu().numpy()
        res.pose = [ground_pose(self.Q, int(r[0]), int(r[1]), self.height) if r[1] > 0 else None for r in rec]
        res.points = free_space_points(self.Q, row, dsp, XR, XT)
        if from_numpy:
            res.ground, res.free_row, res.free_disp = rec, row, dsp
            res.vdisp = None if res.vdisp is None else res.vdisp.cpu().numpy()
            res.labels = None if res.labels is None else res.labels.cpu().numpy()
        return res

    def objects(self, left, right, pixel_format="bgr", transform=None, capacity=64, positions=True, **spec):
        """What stands on the ground, as boxes with a 3-D position each and without a detector, for B pairs: front end, engine,
        engine.ground_from_disparity (labels only), engine.stixels_from_disparity on the float disparity and those labels and, with
        positions, engine.box_positions_from_disparity(select="near", disparity="d1") on the boxes and counts as they lie on the device -
        nothing dense crosses the host link and nothing is waited for.  spec: the words of ground_from_disparity (vh_lo, vh_hi, vh_step,
        qb_step, tol, g_tol, min_run, min_support) and of stixels_from_disparity (q_min, sim, max_gap, min_rows, max_layers, col_step,
        sim_cols, min_cols); the bins follow the rig's disp_max.  -> engine.StixelResult with boxes, info int32 [B,capacity,4], counts
        int32 [B] (not capped by the capacity), n_stixels, stixels, positions float64 [B,capacity,3] in metres (NaN at and beyond
        counts[b]; None without positions), stat (box_positions' int32 [B,capacity,4]) and ground (the GroundResult).  transform as in
        top_view: None (camera axes), "rig" or (XR, XT).  CUDA input: device tensors; numpy input: numpy arrays."""
        if self.params.subsampling:
            raise ValueError("objects does not support half-resolution maps (params.subsampling)")
        if "disp_max" in spec or "n_bins" in spec:
            raise ValueError("objects: disp_max and n_bins are not options of the rig (the bins follow the rig's disp_max)")
        words = ("q_min", "sim", "max_gap", "min_rows", "max_layers", "col_step", "sim_cols", "min_cols")
        mine = {k: spec.pop(k) for k in words if k in spec}
        if spec.get("min_support") is None:
            spec["min_support"] = self.width
        ground_spec(self.height, self.params.disp_max, **spec)  # argument errors before any work
        stixel_spec(self.params.disp_max, **mine)
        if isinstance(capacity, bool) or int(capacity) != capacity or not 0 <= capacity <= 65535:
            raise ValueError("capacity must be an integer in 0 .. 65535, got %r" % (capacity,))
        XR, XT = self._transform(transform)
        gl, gr, _, from_numpy = self._run_frontend(left, right, pixel_format, False)
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        g = ground_from_disparity(d1, self.params.disp_max, want_vdisp=False, want_free=False, **spec)
        res = stixels_from_disparity(d1, g.labels, self.params.disp_max, capacity=int(capacity), **mine)
        res.ground = g
        if positions and capacity == 0:  # no row to fill, and an empty tensor has no address to give
            res.positions, res.stat = res.boxes.new_empty((d1.shape[0], 0, 3)).double(), res.boxes.new_empty((d1.shape[0], 0, 4))
        elif positions:
            res.positions, res.stat = box_positions_from_disparity(d1, self.Q, res.boxes, res.counts, XR=XR, XT=XT, select="near", disparity="d1")
        if from_numpy:
            for k in ("stixels", "n_stixels", "boxes", "info", "counts", "positions", "stat"):
                t = getattr(res, k)
                setattr(res, k, None if t is None else t.cpu().numpy())
            g.ground, g.labels = g.ground.cpu().numpy(), g.labels.cpu().numpy()
        return res

    def occupancy(self, left, right, x_range, y_range, z_range, scale, pixel_format="bgr", transform=None, ground=None, **spec):
        """Occupancy and elevation grids of B pairs - what a planner takes: front end, engine, engine.ground_from_disparity (labels and
        free space; `ground`: a dict of its spec words vh_lo, vh_hi, vh_step, qb_step, tol, g_tol, min_run, min_support, or None) and
        engine.occupancy_from_disparity on the float disparity, all on the device - nothing dense crosses the host link and nothing is
        waited for.  The grid is top_view's (x_range, y_range, z_range, scale) in the frame of `transform` (as in top_view: None - camera
        axes -, "rig" or (XR, XT); a vehicle grid takes (CAMERA_TO_VEHICLE, None)); spec: z_scale, min_obstacle, min_ground, min_rays,
        want_state as there.  -> engine.OccupancyResult with cells, n_rays, state and ground (the GroundResult).  CUDA input: device
        tensors; numpy input: numpy arrays."""
        if self.params.subsampling:
            raise ValueError("occupancy does not support half-resolution maps (params.subsampling)")
        gspec = dict(ground or {})
        if any(k in gspec for k in ("want_free", "want_labels", "want_vdisp", "disp_max", "n_bins")):
            raise ValueError("occupancy: ground takes the spec words of ground_from_disparity only (labels and free space are always computed, the bins follow the rig's disp_max)")
        if gspec.get("min_support") is None:
            gspec["min_support"] = self.width
        XR, XT = self._transform(transform)
        ground_spec(self.height, self.params.disp_max, **gspec)  # argument errors before any work
        occupancy_spec(x_range, y_range, z_range, scale, XT=XT, **{k: v for k, v in spec.items() if k != "want_state"})
        gl, gr, _, from_numpy = self._run_frontend(left, right, pixel_format, False)
        d1, _ = self.engine.process_device(gl, gr, want_d2=False)
        g = ground_from_disparity(d1, self.params.disp_max, want_vdisp=False, **gspec)
        res = occupancy_from_disparity(d1, g.labels, g.free_row, g.free_disp, self.Q, x_range, y_range, z_range, scale, XR=XR, XT=XT, **spec)
        res.ground = g
        if from_numpy:
            for obj, names in ((res, ("cells", "n_rays", "state")), (g, ("ground", "labels", "free_row", "free_disp"))):
                for k in names:
                    t = getattr(obj, k)
                    setattr(obj, k, None if t is None else t.cpu().numpy())
        return res

    def occupancy_map(self, x_range, y_range, scale, **log_odds_words):
        """-> OccupancyMap: a world-fixed log-odds map on the rig's device, to be fed with occupancy()'s results and the poses of the
        caller's odometry."""
        return OccupancyMap(x_range, y_range, scale, device=self.device, **log_odds_words)


    def voxel_map(self, lo, hi, size, capacity):
        """-> VoxelMap: a world-fixed voxel map on the rig's device, to be fed with voxel_clouds' or compact_clouds' rows and the poses of
        the caller's odometry."""
        return VoxelMap(lo, hi, size, capacity, device=self.device)

    def place_index(self, r_max, capacity=1024, **words):
        """-> PlaceIndex: a database of places on the rig's device, to be fed with the voxel rows of keyframes and their poses; words:
        stereo_vision.sv.place_params' rings, sectors, z_lo, z_hi and r_min."""
        return PlaceIndex(_sv.place_params(r_max, **words), capacity, device=self.device)

    def pose_graph(self, capacity=1024):
        """-> PoseGraph: the pose graph of a drive on the rig's device: add_chain(odometry's poses), add_loop per confirmed loop,
        optimize(), and corrections() into VoxelMap.repose and PlaceIndex.repose."""
        return PoseGraph(capacity, device=self.device)

    def render_camera(self, size, footprint=1.0):
        """-> the camera VoxelMap.render draws into, from the rig's own Q, width and height and the map's voxel size
        (stereo_vision.sv.voxel_render_camera): `m.render(poses, rig.render_camera(m.params["size"]), transform=..., measured=d1)` is
        the idiom.  footprint: the edge of a voxel's square in voxels."""
        return _sv.voxel_render_camera(self.Q, self.width, self.height, size, footprint)


class VoxelMap:
    """A world-fixed voxel map (include/stereo_vision_hip.h (Q), stereo_vision.sv.voxel_map_insert / voxel_map_rows): per cubic cell of
    edge `size` of the box lo .. hi (metres, world axes) the integer sums of the rows that fell into it, for at most `capacity` voxels.
    device: a CUDA device ("cuda", "cuda:1", an index) - engine.voxel_map_insert, one kernel per update, and engine.voxel_map_rows - or
    "cpu" - the numpy definition on CPU tensors or numpy arrays, the same methods and the same bits.  params is the map's
    sv_voxel_map_spec as a dict, seq the number of frames added so far: the sequence number the next frame carries.  match() and localize()
    are group (R): a frame's rows scored against the map at candidate poses, and the best pose of a window around a guess - localize, then
    update at the refined pose.  prune(), recenter(), resize() and merge() are group (S), stereo_vision.sv.voxel_map_carry: the map's voxels,
    filtered and shifted by whole cells, carried into an empty table - fewer voxels, a box that follows the vehicle, a larger capacity -
    or another map's voxels added to this one.  The first three carry into a spare buffer of the map's size, allocated on first use and
    swapped with the map's from then on: they double the memory the map takes and allocate once, not per call.  carve() is group (T),
    stereo_vision.sv.voxel_map_carve: the voxels that the sight lines of later frames pass through are emptied, and keep their slots until
    the next prune().  render() is group (U), stereo_vision.sv.voxel_map_render: what a camera should see of the map from given poses -
    depth, colour and expected disparity per pixel - and, against a measured disparity, what is new and what was seen through.
    flatten() is group (V), stereo_vision.sv.voxel_map_flatten: the voxels sliced by height above the floor and written out as the
    logodds and last_seen of a flat map, which OccupancyMap.load_voxels takes.  clusters() and despeckle() are group (W),
    stereo_vision.sv.voxel_map_clusters: the connected components of the voxels - a row of counts, sums and a box per object, a label per
    voxel - and the components below a size emptied.  align() is group (X), stereo_vision.sv.voxel_map_align: a frame's pose refined by
    iterative closest point against the voxels' means, below localize's step and in roll and pitch as well.  normals() is group (Y),
    stereo_vision.sv.voxel_map_normals: a plane per voxel through the means around it, which align(method="plane") fits the rows to.
    repose() and merge(pose=...) are group (AD), stereo_vision.sv.voxel_map_repose: the voxels moved by the rigid correction of the frame
    that saw them last - the corrected poses of a loop closure applied to the map - or another map's voxels taken in under one rigid
    transform."""

    def __init__(self, lo, hi, size, capacity, device="cuda"):
        import torch
        self.params = _sv.voxel_map_params(lo, hi, size, capacity)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.seq = 0
        self._spare = None  # prune()'s, recenter()'s and resize()'s second buffer, made on first use
        self._miss = None   # carve()'s word per slot, made on first use
        self._clusters = None  # clusters()' result and workspace, made on first use
        self._normals, self._normals_fresh = None, False  # normals()' (arguments, result), and whether the map is still the one it describes
        if self.device.type == "cuda":
            self.buffer, self._state = voxel_map_new(self.params, self.device), None
        else:
            self.buffer, self._state = None, _sv.voxel_map_state(self.params)

    def reset(self):
        """An empty map: no voxel, dropped 0, not overflowed, seq 0."""
        if self._state is None:
            voxel_map_clear(self.buffer, self.params)
        else:
            self._state = _sv.voxel_map_state(self.params)
        self.seq = 0
        self._stale()

    def update(self, xyz, color, n, counts, poses):
        """Adds B frames: xyz float32 or float64 [B,cap,3], color uint8 [B,cap,4] or None, n int32 [B,cap] or None (every weight 1), counts
        int32 [B] - StereoRig.voxel_clouds' or compact_clouds' tensors on the map's device -, poses float64 [B,12]
        (stereo_vision.sv.voxel_map_pose) or the occupancy map's [B,4] (occupancy_pose), numpy or a tensor.  The frames are numbered on
        from the last call.  Not waited for."""
        import torch
        if self._state is None:
            voxel_map_insert(self.buffer, self.params, xyz, color, n, counts, poses, self.seq)
        else:
            host = [None if t is None else (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for t in (xyz, color, n, counts, poses)]
            host[4] = _sv.voxel_map_pose_words(host[4])
            _sv.voxel_map_insert(self._state, *host, seq0=self.seq)
        self.seq += int(xyz.shape[0])
        self._stale()

    def rows(self, min_n=1, min_rows=1, since=0, dtype="f32"):
        """The voxels with n >= min_n, m >= min_rows rows and last_seq >= since, in ascending key, as a dict of tensors on the map's
        device: xyz [V,3], color uint8 [V,4], cell int32 [V,3], n, m int64 [V], first_seq, last_seq int32 [V], key int64 [V], and count
        (an int; -1 and no rows for an overflowed map).  Reads the count back."""
        import torch
        if self._state is None:
            return voxel_map_rows(self.buffer, self.params, min_n, min_rows, since, dtype, sort=True)
        res = _sv.voxel_map_rows(self._state, min_n, min_rows, since, dtype)
        return {k: v if k == "count" else torch.from_numpy(v) for k, v in res.items()}

    def match(self, xyz, n, counts, poses, min_n=1, min_rows=1, since=0):
        """Scores B frames against the map as it stands (include/stereo_vision_hip.h (R), stereo_vision.sv.voxel_map_match): xyz, n and
        counts as for update, poses float64 [B,P,12] (stereo_vision.sv.voxel_map_pose), numpy or a tensor - frame b's own P candidates.
        A row hits where its cell holds a voxel with n >= min_n, m >= min_rows and last_seq >= since.  -> engine.VoxelMatchResult with
        inside, hits, weight, d2 [B,P] and best, best_weight, best_d2 [B] as tensors on the map's device.  The map is not changed; not
        waited for."""
        import torch
        from .engine import VoxelMatchResult
        if self._state is None:
            return voxel_map_match(self.buffer, self.params, xyz, n, counts, poses, min_n, min_rows, since)
        host = [None if t is None else (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for t in (xyz, n, counts, poses)]
        res = _sv.voxel_map_match(self._state, *host, min_n=min_n, min_rows=min_rows, since=since)
        return VoxelMatchResult(**{k: torch.from_numpy(np.ascontiguousarray(res[k])) for k in VoxelMatchResult.__slots__})

    def localize(self, xyz, n, counts, guess_xyzyaw, half, steps, min_n=1, min_rows=1, since=0):
        """The best pose per frame of a window around its guess: guess_xyzyaw float64 [B,4] = (x, y, z, yaw) ([4] for one frame), half =
        (dx, dy, dz, dyaw) and steps = (nx, ny, nz, nyaw) as stereo_vision.sv.voxel_map_pose_window takes them - the guess is candidate 0
        and keeps ties.  -> (float64 numpy [B,4], the refined (x, y, z, yaw); the VoxelMatchResult).  Waits for the best indices - B words
        - and reads nothing else back; a frame whose best is -1 (an overflowed map) keeps its guess."""
        g = np.asarray(guess_xyzyaw, np.float64)
        g = g[None] if g.ndim == 1 else g
        if g.shape != (int(xyz.shape[0]), 4):
            raise ValueError("localize: guess_xyzyaw must be [%d,4], got %s" % (int(xyz.shape[0]), g.shape))
        window = np.stack([_sv.voxel_map_pose_window(x, y, z, yaw, half, steps) for x, y, z, yaw in g]) if len(g) else np.zeros((0, 1, 4))
        res = self.match(xyz, n, counts, _sv.voxel_map_pose(window[..., 0], window[..., 1], window[..., 3], window[..., 2]), min_n, min_rows, since)
        best = res.best.cpu().numpy().astype(np.int64)
        return window[np.arange(len(g)), np.maximum(best, 0)], res  # row 0 is the guess

    def normals(self, m=16, min_nb=5, flat=64, wide=16, **filters):
        """The surface normals of the voxels (include/stereo_vision_hip.h (Y), stereo_vision.sv.voxel_map_normals): per voxel the plane
        through the means of the voxels around it, as the best of the 2 m^2 + 1 directions of stereo_vision.sv.voxel_normal_dirs(m); a
        voxel with fewer than min_nb neighbours, on a pole or an edge, or in a blob gets none (flat, wide: the thresholds, in 1/256).
        filters: min_n, min_rows, since.  -> engine.VoxelNormalsResult on the device - normal int32 per slot, counts, dirs, not waited
        for -, or on "cpu" the definition's dict with normal per entry in ascending key.  The map keeps the result, and
        align(method="plane") uses it until update, an applied carve, despeckle, prune, recenter, resize or merge has changed the map."""
        from .engine import voxel_map_normals
        f = self._filters(filters)
        asked = (int(m), int(min_nb), int(flat), int(wide)) + tuple(int(v) for v in f)
        dirs = _sv.voxel_normal_dirs(m)
        if self._state is None:
            keep = self._normals[1] if self._normals is not None else None
            if keep is not None and keep.normal.numel() != _sv.voxel_map_slots(self.params["capacity"]):
                keep = None  # of the map before a resize
            if keep is not None and self._normals[0][0] == asked[0]:
                dirs = keep.dirs  # the table is already on the device
            res = voxel_map_normals(self.buffer, self.params, dirs, min_nb, flat, wide, *f, out=keep)
        else:
            res = _sv.voxel_map_normals(self._state, dirs, min_nb, flat, wide, *f)
        self._normals, self._normals_fresh = (asked, res), True
        return res

    def _stale(self):
        """The map has changed: what normals() kept no longer describes it."""
        self._normals_fresh = False

    def align(self, xyz, n, counts, poses, iterations=10, max_dist=1.0, dof=6, min_pairs=6, eps=None, min_n=1, min_rows=1, since=0, method="point"):
        """Refines one pose per frame by iterative closest point against the map as it stands (include/stereo_vision_hip.h (X),
        stereo_vision.sv.voxel_map_align): xyz, n and counts as for update, poses float64 [B,12] or [B,4] - the start: localize's best,
        or the odometry's.  Per round every row is paired with the nearest voxel mean within max_dist cells and the pairs are fitted in
        closed form: dof=6 all of the rotation and the translation, dof=4 yaw and the translation.  -> (float64 numpy [B,12], the
        refined poses; engine.VoxelAlignResult with sums, poses, ok, rounds, pairs and rms).  A frame the last round could not fit (ok
        False: fewer than min_pairs pairs, an overflowed map) keeps the pose it had.  Waits once per round, for B x 19 words.  The idiom:
        g, _ = vm.localize(...); poses, _ = vm.align(xyz, n, counts, sv.voxel_map_pose(g[:, 0], g[:, 1], g[:, 3], g[:, 2]));
        vm.update(xyz, color, n, counts, poses).  The map is not changed.  method="plane" (group (Y)) fits the rows to the planes of
        normals() instead of to the voxels' means, which lets a row slide along the road or the wall it lies on: a few rounds where
        "point" takes many; it uses the normals the map keeps and fits them again - as normals() was last called, or with its defaults
        and these filters - where the map has changed since.  -> (poses, engine.VoxelPlaneResult)."""
        import torch
        from .engine import VoxelAlignResult, VoxelPlaneResult
        if method not in _sv.VOXEL_ALIGN_METHODS:
            raise ValueError("method must be 'point' or 'plane', got %r" % (method,))
        kept = None
        if method == "plane":
            if not self._normals_fresh:
                if self._normals is None:
                    self.normals(min_n=min_n, min_rows=min_rows, since=since)
                else:
                    m, min_nb, flat, wide, f0, f1, f2 = self._normals[0]
                    self.normals(m, min_nb, flat, wide, min_n=f0, min_rows=f1, since=f2)
            kept = self._normals[1]
        if self._state is None:
            res = voxel_map_align(self.buffer, self.params, xyz, n, counts, poses, iterations, max_dist, dof, min_pairs, eps, min_n, min_rows, since, method, kept)
            return res.poses, res
        host = [None if t is None else (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for t in (xyz, n, counts, poses)]
        got = _sv.voxel_map_align(self._state, *host, iterations=iterations, max_dist=max_dist, dof=dof, min_pairs=min_pairs, eps=eps, min_n=min_n,
                                  min_rows=min_rows, since=since, method=method, normals=kept)
        res = (VoxelAlignResult if method == "point" else VoxelPlaneResult)(**dict(got, sums=torch.from_numpy(got["sums"])))
        return res.poses, res

    def stats(self):
        """{"claimed", "dropped", "overflowed"}: the voxels the map holds, the rows it dropped, whether it ever held more than its
        capacity.  The one read-back of the map's head."""
        if self._state is None:
            claimed, dropped, overflowed = voxel_map_stats(self.buffer)
        else:
            claimed, dropped, overflowed = len(self._state["key"]), self._state["dropped"], self._state["overflowed"]
        return {"claimed": int(claimed), "dropped": int(dropped), "overflowed": bool(overflowed)}

    @staticmethod
    def _filters(filters):
        """min_n, min_rows, since of a carry, from the keywords of a method."""
        unknown = set(filters) - {"min_n", "min_rows", "since"}
        if unknown:
            raise TypeError("unknown filter %s: min_n, min_rows and since are the filters" % sorted(unknown))
        return filters.get("min_n", 1), filters.get("min_rows", 1), filters.get("since", 0)

    def _carry_over(self, params, shift, filters):
        """The map's voxels, filtered and shifted, carried into an empty map of `params`, which becomes the map; -> the counts."""
        f = self._filters(filters)
        self._stale()
        if self._state is not None:
            state = _sv.voxel_map_state(params)
            stats = _sv.voxel_map_carry(state, self._state, shift, *f)
            self._state, self.params = state, state["params"]
            return stats
        same = params["capacity"] == self.params["capacity"]
        if same and self._spare is None:
            self._spare = voxel_map_new(params, self.device)
        into = voxel_map_clear(self._spare, params) if same else voxel_map_new(params, self.device)
        stats = voxel_map_carry(into, params, self.buffer, self.params, shift, *f)
        if same:
            self.buffer, self._spare = into, self.buffer
        else:
            self.buffer, self._spare = into, None  # the old pair goes back to torch's allocator, behind the kernels of this stream
        self.params = params
        return stats

    def repose(self, corr, seq0=0, params=None, **filters):
        """Re-poses the map after a loop closure (include/stereo_vision_hip.h (AD), stereo_vision.sv.voxel_map_repose): every voxel is moved
        by the rigid correction of the frame that saw it last - corr float64 [K,12], numpy or a tensor on the map's device, what
        stereo_vision.sv.pose_corrections makes of the drive's poses and the corrected ones; the correction of a voxel is corr[min(max(
        last_seq - seq0, 0), K - 1)] - and accumulated into an empty table, which becomes the map: the spare buffer, as prune() uses
        it.  params: a new box and capacity (stereo_vision.sv.voxel_map_params' dict; the size may differ too) for corrections that move
        the map's extent; None keeps the map's.  filters: min_n, min_rows, since prune on the way.  A re-pose costs up to 1 / 65536 of a
        cell of position: a voxel's points collapse to their mean.  seq stays; what normals() kept is stale.  -> the counts, as
        prune()."""
        f = self._filters(filters)
        params = self.params if params is None else _sv.voxel_map_params(params["lo"], params["hi"], params["size"], params["capacity"])
        self._stale()
        if self._state is not None:
            corr = corr.cpu().numpy() if hasattr(corr, "cpu") else corr
            state = _sv.voxel_map_state(params)
            stats = _sv.voxel_map_repose(state, self._state, corr, seq0, *f)
            self._state, self.params = state, state["params"]
            return stats
        same = params["capacity"] == self.params["capacity"]
        if same and self._spare is None:
            self._spare = voxel_map_new(params, self.device)
        into = voxel_map_clear(self._spare, params) if same else voxel_map_new(params, self.device)
        stats = voxel_map_repose(into, params, self.buffer, self.params, corr, seq0, *f)
        if same:
            self.buffer, self._spare = into, self.buffer
        else:
            self.buffer, self._spare = into, None  # the old pair goes back to torch's allocator, behind the kernels of this stream
        self.params = params
        return stats

    def prune(self, min_n=1, min_rows=1, since=0):
        """Forgets: keeps the voxels with n >= min_n, m >= min_rows and last_seq >= since - rows()' filters - in the same box and
        capacity, with every sum as it was.  -> the counts carried, filtered, outside, claimed (stereo_vision.sv.VOXEL_CARRY_STATS): an
        int64 [4] tensor on the device, not waited for, or a dict on "cpu".  seq stays."""
        return self._carry_over(self.params, (0, 0, 0), dict(min_n=min_n, min_rows=min_rows, since=since))

    def recenter(self, x, y, z=None, **filters):
        """Scrolls the box by whole cells so that the world point (x, y, z) lies in its middle cell
        (stereo_vision.sv.voxel_map_recenter_shift; z = None leaves the z axis alone); params becomes voxel_map_shifted's, the voxels
        that leave the box are lost - counted as outside - and the filters min_n, min_rows, since prune on the way.  Nothing is done, and
        zeros are returned, where the box does not move and no filter is given.  -> the counts, as prune()."""
        import torch
        k = _sv.voxel_map_recenter_shift(self.params, x, y, z)
        if k == (0, 0, 0) and not filters:
            self._filters(filters)
            zeros = dict.fromkeys(_sv.VOXEL_CARRY_STATS, 0)
            return zeros if self._state is not None else torch.zeros((4,), dtype=torch.int64, device=self.device)
        most = _sv.VOXEL_CARRY_SHIFT_MAX  # an axis has at most that many cells: a longer way carries nothing either
        return self._carry_over(_sv.voxel_map_shifted(self.params, k), tuple(max(-most, min(most, -v)) for v in k), filters)

    def resize(self, capacity, **filters):
        """A new capacity in the same box: the way out before an overflow, when stats()["claimed"] nears the capacity (an overflowed map
        stays lost).  The filters prune on the way.  -> the counts, as prune()."""
        return self._carry_over(_sv.voxel_map_params(self.params["lo"], self.params["hi"], self.params["size"], capacity), (0, 0, 0), filters)

    def merge(self, other, pose=None, **filters):
        """Adds the voxels of `other` - those that pass the filters and lie in this map's box - to this map; `other` is not changed.  With
        pose float64 [12] (stereo_vision.sv.voxel_map_pose's layout) the other map's voxels come in under that one rigid transform, from
        other's world into this one's (group (AD), stereo_vision.sv.voxel_map_repose with K = 1): two sessions or ranks whose frames
        differ by more than whole cells; the maps may then differ in box, size and capacity, and each voxel comes in as one row at its
        mean.  Without a pose (group (S)) both maps lie on one device and have the same size, and other's box must start a whole number of cells from this one's: the shift is
        round((other.lo - self.lo) / size), and ValueError is raised where that quotient misses it by more than
        stereo_vision.sv.VOXEL_MERGE_TOLERANCE = 1 / 65536 of a cell - the unit of the sub-cell offsets the voxels hold: a box that is
        off by less displaces no point by more than the map resolves, and the roundings voxel_map_shifted leaves in lo are smaller by
        orders of magnitude; a box that is off by more needs resampling, which this is not.  seq becomes the larger of the two.  -> the
        counts, as prune()."""
        f = self._filters(filters)
        if not isinstance(other, VoxelMap) or other is self or other.device != self.device:
            raise ValueError("merge needs another VoxelMap on %s" % (self.device,))
        if pose is not None:
            corr = np.ascontiguousarray(pose.cpu().numpy() if hasattr(pose, "cpu") else pose, np.float64)
            if corr.shape != (12,):
                raise ValueError("merge: pose must be float64 [12], got shape %s" % (corr.shape,))
            if self._state is not None:
                stats = _sv.voxel_map_repose(self._state, other._state, corr[None], 0, *f)
            else:
                stats = voxel_map_repose(self.buffer, self.params, other.buffer, other.params, corr[None], 0, *f)
            self.seq = max(self.seq, other.seq)
            self._stale()
            return stats
        size = np.float64(self.params["size"])
        if np.float64(other.params["size"]).tobytes() != size.tobytes():
            raise ValueError("merge needs maps of one size, got %r and %r" % (self.params["size"], other.params["size"]))
        t = (np.array(other.params["lo"]) - np.array(self.params["lo"])) / size
        shift = np.rint(t)
        if not (np.abs(t - shift) <= _sv.VOXEL_MERGE_TOLERANCE).all() or not (np.abs(shift) <= _sv.VOXEL_CARRY_SHIFT_MAX).all():
            raise ValueError("merge: the box of the other map does not start a whole number of cells (at most 2^20) from this one's: %r cells" % (t.tolist(),))
        shift = tuple(int(v) for v in shift)
        if self._state is not None:
            stats = _sv.voxel_map_carry(self._state, other._state, shift, *f)
        else:
            stats = voxel_map_carry(self.buffer, self.params, other.buffer, other.params, shift, *f)
        self.seq = max(self.seq, other.seq)
        self._stale()
        return stats

    def carve(self, xyz, n, counts, poses, origin=None, seq0=None, reach_m=20.0, margin=1, min_miss=2, ratio=0, apply=True, prune=False):
        """Un-sees: carves free space out of the map along the sight lines of B frames (include/stereo_vision_hip.h (T),
        stereo_vision.sv.voxel_map_carve).  xyz, n, counts and poses as for update; seq0 the sequence number of frame 0, None = seq - B:
        the frames update() has just added, so that `m.update(xyz, color, n, counts, poses); m.carve(xyz, n, counts, poses)` is the
        idiom - a voxel those frames (or later ones) have seen is never counted against.  origin: the sensor's centre in the frame's
        axes (None: 0, 0, 0).  A kept row casts a ray from the sensor's cell if its own cell lies within reach = ceil(reach_m / size)
        cells of it (ValueError above 1023); the last `margin` cells in front of the row's are left alone; a voxel with at least min_miss
        weight of rays through it, and at least ratio / 256 of its own weight, is emptied under `apply`.  An emptied voxel keeps its slot
        until the next prune() - prune=True follows with one -: stats()["claimed"] does not change, every method skips it at min_n >= 1,
        and rows() is defined for min_n >= 1 only until then.  -> engine.VoxelCarveResult (stats int64 [4] = rays, steps, touched,
        carved, and the per-slot miss tensor, which the map allocates once and reuses: valid until the next carve) on the device, not
        waited for; on "cpu" the definition's dict.  touched() turns either into (key, miss)."""
        import torch
        from .engine import voxel_carve_miss, voxel_map_carve
        B = int(xyz.shape[0])
        seq0 = self.seq - B if seq0 is None else seq0
        reach = int(np.ceil(np.float64(reach_m) / np.float64(self.params["size"]))) if np.isfinite(reach_m) else 0
        if not 1 <= reach <= _sv.VOXEL_CARVE_REACH_MAX:
            raise ValueError("carve: reach_m = %r is %d cells of %r m: 1 .. 1023 cells" % (reach_m, reach, self.params["size"]))
        origin = (0.0, 0.0, 0.0) if origin is None else origin
        if self._state is None:
            if self._miss is None or self._miss.numel() != _sv.voxel_map_slots(self.params["capacity"]):
                self._miss = voxel_carve_miss(self.buffer, self.params)
            res = voxel_map_carve(self.buffer, self.params, xyz, n, counts, poses, origin, seq0, reach, margin, min_miss, ratio, apply, miss=self._miss)
        else:
            host = [None if t is None else (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)) for t in (xyz, n, counts, poses)]
            host[3] = _sv.voxel_map_pose_words(host[3])
            res = _sv.voxel_map_carve(self._state, *host, origin=origin, seq0=seq0, reach=reach, margin=margin, min_miss=min_miss, ratio=ratio, apply=apply)
        if apply:
            self._stale()
        if prune:
            self.prune()
        return res

    def touched(self, result):
        """(key, miss) of the voxels carve() counted rays against, ascending in key: int64 tensors on the map's device.  Call it before
        anything else changes the map - prune() included, so not behind carve(prune=True) -; reads back."""
        import torch
        from .engine import voxel_carve_touched
        if self._state is None:
            return voxel_carve_touched(self.buffer, self.params, result.miss)
        return torch.from_numpy(result["key"]), torch.from_numpy(result["miss"])

    def render(self, poses, camera, transform=None, measured=None, tol=1.0, near=None, far=None, r_max=4, min_n=1, min_rows=1, since=0):
        """What a camera should see of the map from V poses (include/stereo_vision_hip.h (U), stereo_vision.sv.voxel_map_render): poses
        as for update - frame to world, float64 [V,12] or [V,4], numpy or a tensor -, camera StereoRig.render_camera's dict, transform
        the rig's (XR, XT) from the camera's axes to the frame's (None: the frame's axes are the camera's); the world-to-camera words
        are made on the host (stereo_vision.sv.voxel_render_cams).  measured: float32 [V,H,W] on the map's device - the engine's D1 of
        the frames at those poses - to compare the expected disparity with, at tol pixels.  near, far in cells (None: 1 and 2^20), r_max
        in pixels, min_n >= 1, min_rows, since: rows()' filters.  -> engine.VoxelRenderResult - depth, key, color, disparity, stats, and
        with measured label and counts - of tensors on the map's device.  The map is not changed; not waited for."""
        import torch
        from .engine import VoxelRenderResult, voxel_map_render
        p = poses.cpu().numpy() if isinstance(poses, torch.Tensor) else poses
        XR, XT = (None, None) if transform is None else transform
        cams = _sv.voxel_render_cams(p, XR, XT)
        if self._state is None:
            return voxel_map_render(self.buffer, self.params, cams, camera, measured, tol, near, far, r_max, min_n, min_rows, since)
        m = measured.cpu().numpy() if isinstance(measured, torch.Tensor) else measured
        res = _sv.voxel_map_render(self._state, cams, camera, m, tol, near, far, r_max, min_n, min_rows, since)
        return VoxelRenderResult(**{k: None if v is None else torch.from_numpy(v) for k, v in res.items()})

    def flatten(self, flat_map, z_ref=None, step=0.2, height=2.0, radius=2, min_obstacle=1, min_ground=1, min_n=1, min_rows=1, since=0, out=None):
        """The map sliced by height and written out in a flat map's layout (include/stereo_vision_hip.h (V),
        stereo_vision.sv.voxel_map_flatten): flat_map an OccupancyMap or the dict of a flat map's words
        (stereo_vision.sv.occupancy_map_params); z_ref the height of the floor in the world, metres, or None for the local floor - per
        flat cell the lowest voxel within `radius` cells; a voxel less than `step` metres from the floor is ground, one below `height`
        metres an obstacle, one above it overhead - a bridge, a crown - and no obstacle; a cell is occupied from min_obstacle obstacle
        voxels on, else free from min_ground ground voxels on, else unknown; min_n >= 1, min_rows, since: rows()' filters.  out: an
        engine.VoxelFlattenResult to write into.  -> engine.VoxelFlattenResult - logodds, last_seen, floor, top, cells, stats - of
        tensors on the map's device.  The map is not changed; not waited for.  OccupancyMap.load_voxels puts the result into a flat map."""
        import torch
        from .engine import VoxelFlattenResult, voxel_map_flatten
        words = flat_map.words if isinstance(flat_map, OccupancyMap) else flat_map
        spec = _sv.voxel_flatten_params(self.params, z_ref, step, height, radius, min_obstacle, min_ground)
        if self._state is None:
            return voxel_map_flatten(self.buffer, self.params, words, spec, min_n, min_rows, since, out=out)
        res = _sv.voxel_map_flatten(self._state, words, spec, min_n, min_rows, since)
        return VoxelFlattenResult(**{k: torch.from_numpy(v) for k, v in res.items()})

    def clusters(self, connectivity=26, min_voxels=1, capacity=1024, z_ref=None, h_lo=None, h_hi=None, flat=None, flat_map=None, floor=None, min_n=1, min_rows=1,
                 since=0, drop=False, sort=True):
        """The connected components of the map (include/stereo_vision_hip.h (W), stereo_vision.sv.voxel_map_clusters): the objects in
        it.  connectivity 6, 18 or 26; a component of at least min_voxels voxels gets a row, `capacity` rows at most.  Without a floor
        the heights count from z_ref (metres in the world; None: the box's floor) and the band h_lo .. h_hi, metres, None = open, says
        which voxels take part.  With a floor - flat = an engine.VoxelFlattenResult of flatten() together with flat_map = the flat map it
        was made for, or flat = an OccupancyMap that load_voxels() has just filled, or flat_map and floor themselves - the heights count
        from that floor plane and the band defaults to 0.2 .. 2.0 m, the flatten's obstacle voxels, so that the ground does not glue the
        things that stand on it into one piece.  min_n >= 1, min_rows, since: rows()' filters.  drop: despeckle().  -> an
        engine.VoxelClusterResult - clusters int64 [R,16], info int64 [8], label int32 per slot - on the device, whose tensors the map
        keeps and the next call writes again; on "cpu" the definition's dict as tensors, with label per entry in ascending key.
        engine.voxel_cluster_labels / voxel_cluster_boxes read either.  sort=True waits for one word; sort=False (device only) for
        nothing."""
        import torch
        from .engine import VoxelFlattenResult, voxel_map_clusters
        if isinstance(flat, OccupancyMap):
            if flat._flatten is None:
                raise ValueError("clusters: flat is an OccupancyMap that load_voxels() has not filled")
            flat_map, floor = flat.words, flat._flatten.floor
        elif isinstance(flat, VoxelFlattenResult):
            if flat_map is None:
                raise ValueError("clusters: a flatten result needs flat_map, the flat map it was made for")
            floor = flat.floor
        elif flat is not None:
            raise ValueError("clusters: flat must be an engine.VoxelFlattenResult or an OccupancyMap")
        if isinstance(flat_map, OccupancyMap):
            flat_map = flat_map.words
        mode = 0 if floor is None else 1
        spec = _sv.voxel_cluster_params(self.params, connectivity, min_voxels, capacity, mode, z_ref, h_lo, h_hi, drop)
        if self._state is None:
            self._clusters = voxel_map_clusters(self.buffer, self.params, flat_map=flat_map, floor=floor, min_n=min_n, min_rows=min_rows, since=since, sort=sort,
                                                out=self._clusters, spec=spec)
            return self._clusters
        fl = floor.cpu().numpy() if isinstance(floor, torch.Tensor) else floor
        res = _sv.voxel_map_clusters(self._state, spec, flat_map, fl, min_n, min_rows, since)
        return {k: torch.from_numpy(v) for k, v in res.items()}

    def despeckle(self, min_voxels, connectivity=26, prune=False, **filters):
        """The speckle filter in three dimensions: every voxel of a connected component of fewer than min_voxels voxels is emptied - the
        floating islands that mismatches leave, which no later sight line may ever cross.  filters: min_n, min_rows, since, which say
        what counts as a voxel here.  An emptied voxel keeps its slot until the next prune() - prune=True follows with one -:
        stats()["claimed"] does not change, and every method skips it at min_n >= 1.  -> the info words of clusters(): int64 [8] on the
        device, not waited for (info[4] = the voxels emptied), or a tensor on "cpu"."""
        f = self._filters(filters)
        res = self.clusters(connectivity, min_voxels, 1, min_n=f[0], min_rows=f[1], since=f[2], drop=True, sort=False if self._state is None else True)
        self._stale()
        if prune:
            self.prune()
        return res.info if self._state is None else res["info"]

    def write_ply(self, path, min_n=1, min_rows=1, since=0):
        """rows(...) as a binary PLY of coloured points (stereo_vision.sv.write_ply); -> the number of points.  RuntimeError for an
        overflowed map."""
        res = self.rows(min_n, min_rows, since)
        if res["count"] < 0:
            raise RuntimeError("the voxel map overflowed its capacity of %d voxels: raise it" % self.params["capacity"])
        _sv.write_ply(path, res["xyz"].cpu().numpy(), res["color"].cpu().numpy())
        return res["count"]


class PlaceIndex:
    """A growing database of places (include/stereo_vision_hip.h (AC), stereo_vision.sv.place_descriptor / place_match): per keyframe its
    polar height descriptor, ring key, words, sequence number and pose, on `device` - a CUDA device ("cuda", "cuda:1", an index):
    engine.place_descriptor and engine.place_match -, or "cpu": the numpy definitions on CPU tensors, the same methods and the same bits.
    params: stereo_vision.sv.place_params' dict; capacity: the keyframes the tensors hold at first - add() doubles it by one copy when it
    runs out.  count is the number of keyframes; desc, ring, words, seq and poses are the tensors, of which the first count rows are
    used.  guess() gives the start VoxelMap.localize, then .align, refine; the refined pose becomes a loop edge of a PoseGraph, and
    repose() takes the corrections PoseGraph.corrections() - or stereo_vision.sv.loop_spread - arrives at, as VoxelMap.repose does."""

    def __init__(self, params, capacity, device="cuda"):
        import torch
        self.params = _sv.place_params(params["r_max"], params["rings"], params["sectors"], params["z_lo"], params["z_hi"], params["r_min"])
        if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= capacity <= _sv.PLACE_KEYS_MAX:
            raise ValueError("capacity must be an integer in 1 .. 2^20, got %r" % (capacity,))
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.count = 0
        self._pose_host = np.zeros((0, 12))  # the poses once more, on the host: guess() reads back the best keys only
        self._allocate(int(capacity))

    _FIELDS = ("desc", "ring", "words", "seq", "poses")

    def _allocate(self, capacity):
        import torch
        R, S = self.params["rings"], self.params["sectors"]
        old = [getattr(self, f, None) for f in self._FIELDS]
        self.desc = torch.zeros((capacity, R, S), dtype=torch.uint8, device=self.device)
        self.ring = torch.zeros((capacity, R), dtype=torch.uint8, device=self.device)
        self.words = torch.zeros((capacity, 4), dtype=torch.int32, device=self.device)
        self.seq = torch.zeros((capacity,), dtype=torch.int32, device=self.device)
        self.poses = torch.zeros((capacity, 12), dtype=torch.float64, device=self.device)
        for f, t in zip(self._FIELDS, old):
            if t is not None:
                getattr(self, f)[:self.count].copy_(t[:self.count])
        self.capacity = capacity

    def _on_device(self, t, dtype):
        import torch
        t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
        return t.to(device=self.device, dtype=dtype)

    def _seq(self, seq, B):
        s = np.asarray(seq, np.int64)
        s = s + np.arange(B) if s.ndim == 0 else s
        if s.shape != (B,) or (s < 0).any() or (s > 2 ** 31 - 1).any():
            raise ValueError("seq must be an integer - the first frame's, the others count on - or [%d] of them in 0 .. 2^31 - 1" % B)
        return s.astype(np.int32)

    def descriptor(self, xyz, n, counts, poses=None):
        """The descriptors of B frames of rows - xyz [B,cap,3], n [B,cap] or None, counts [B], as VoxelMap.update takes them, under poses
        [B,12] or None -> {"desc" uint8 [B,R,S], "ring" uint8 [B,R], "words" int32 [B,4]}: tensors on the index's device.  Not waited for."""
        import torch
        res = place_descriptor(xyz, n, counts, self.params, poses)
        return {k: v if isinstance(v, torch.Tensor) else torch.from_numpy(v) for k, v in res.items()}

    def add(self, desc_result, seq, poses):
        """Stores B keyframes: desc_result as descriptor() returns it, seq their sequence numbers ([B], or the first one's), poses float64
        [B,12]: where the vehicle stood (stereo_vision.sv.voxel_map_pose's layout; numpy).  Not waited for."""
        B = int(desc_result["desc"].shape[0])
        p = np.ascontiguousarray(poses, np.float64)
        if p.shape != (B, 12):
            raise ValueError("poses must be float64 [%d,12], got %s" % (B, p.shape))
        s = self._seq(seq, B)
        if self.count + B > _sv.PLACE_KEYS_MAX:
            raise ValueError("an index holds at most 2^20 keyframes")
        if self.count + B > self.capacity:
            self._allocate(min(_sv.PLACE_KEYS_MAX, max(2 * self.capacity, self.count + B)))
        at = slice(self.count, self.count + B)
        self.desc[at], self.ring[at], self.words[at] = (self._on_device(desc_result[k], d) for k, d in (("desc", self.desc.dtype), ("ring", self.ring.dtype), ("words", self.words.dtype)))
        self.seq[at], self.poses[at] = self._on_device(s, self.seq.dtype), self._on_device(p, self.poses.dtype)
        self._pose_host = np.concatenate([self._pose_host, p])
        self.count += B

    def query(self, desc_result, seq, min_gap, ring_gate=-1, max_shift=None, accept=256, want_pair=False):
        """The best keyframe per query (stereo_vision.sv.place_match): desc_result as descriptor() returns it, seq the queries' sequence
        numbers; a keyframe is a candidate if its sequence number is at least min_gap away.  -> {"best" int32 [Q,4] = (key or -1, shift,
        sad, norm), "counts" int32 [Q,3], and with want_pair "pair" int32 [Q,count,2]}: tensors on the index's device.  Not waited for."""
        import torch
        Q, n = int(desc_result["desc"].shape[0]), self.count
        q = [self._on_device(desc_result[k], d) for k, d in (("desc", self.desc.dtype), ("words", self.words.dtype), ("ring", self.ring.dtype))]
        res = place_match(q[0], q[1], q[2], self._on_device(self._seq(seq, Q), self.seq.dtype), self.desc[:n], self.words[:n], self.ring[:n], self.seq[:n], min_gap,
                          ring_gate, max_shift, accept, want_pair)
        return {k: v if isinstance(v, torch.Tensor) else torch.from_numpy(v) for k, v in res.items()}

    def repose(self, corr, seq0=0):
        """The stored key poses after a loop closure: pose r becomes corr[k] o pose r with k = min(max(seq[r] - seq0, 0), K - 1) -
        VoxelMap.repose's index rule on the keys' sequence numbers, by stereo_vision.sv.pose_repose on a read-back copy (96 bytes a
        key) -, so that guess() points into the re-posed map.  corr float64 [K,12], numpy or a tensor.  Reads back the sequence numbers."""
        n = self.count
        corr = corr.cpu().numpy() if hasattr(corr, "cpu") else corr
        moved = _sv.pose_repose(self.poses[:n].cpu().numpy(), self.seq[:n].cpu().numpy(), corr, seq0)
        self.poses[:n] = self._on_device(moved, self.poses.dtype)
        self._pose_host = moved

    def guess(self, result):
        """query()'s result -> (ok bool [Q], xyzyaw float64 [Q,4]): per accepted query the start VoxelMap.localize takes - the key's
        position with its heading turned by the shift (stereo_vision.sv.place_guess) -, NaN where nothing was accepted.  Reads back the
        Q x 4 words of best."""
        best = result["best"].cpu().numpy()
        ok = best[:, 0] >= 0
        out = np.full((len(best), 4), np.nan)
        out[ok] = _sv.place_guess(self._pose_host[best[ok, 0]], best[ok, 1], self.params["sectors"])
        return ok, out


class PoseGraph:
    """The pose graph of a drive (include/stereo_vision_hip.h (AE), stereo_vision.sv.pose_graph_optimize): a pose per frame, the
    odometry edges of the chain and the loop edges PlaceIndex and VoxelMap.localize / .align confirm, on `device` - a CUDA device:
    engine.pose_graph_optimize, every round's linearise and solve in HIP -, or "cpu": the numpy definition, the same methods and the same
    bits.  An edge is checked when it is added and kept twice: on the host, where the loop of rounds reads weights and kinds, and on the
    device - i, j int32, Z float64 [.,12], of which the first n_edges rows are used -, where the kernels read it without another upload.
    Both grow by doubling with one copy; the device's rows are filled by one copy per optimize() for all edges added since the last.
    capacity is what they hold at first."""

    _FIELDS = (("i", np.int32, ()), ("j", np.int32, ()), ("Z", np.float64, (12,)), ("w", np.float64, (2,)), ("kind", np.int32, ()))
    _ON_DEVICE = ("i", "j", "Z")

    def __init__(self, capacity=1024, device="cuda"):
        import torch
        if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= capacity <= _sv.POSE_GRAPH_EDGES_MAX:
            raise ValueError("capacity must be an integer in 1 .. 2^22, got %r" % (capacity,))
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.n_edges, self._sent, self.poses, self.fixed, self.optimized = 0, 0, np.zeros((0, 12)), np.zeros(0, bool), None
        self._host = {}
        self._allocate(int(capacity))

    def _allocate(self, capacity):
        import torch
        for name, dtype, shape in self._FIELDS:
            old = self._host.get(name)
            self._host[name] = np.zeros((capacity,) + shape, dtype)
            if old is not None:
                self._host[name][:self.n_edges] = old[:self.n_edges]
            if name in self._ON_DEVICE:
                was = getattr(self, name, None)
                setattr(self, name, torch.zeros((capacity,) + shape, dtype=torch.from_numpy(self._host[name][:0]).dtype, device=self.device))
                if was is not None:
                    getattr(self, name)[:self._sent].copy_(was[:self._sent])
        self.capacity = capacity

    def _add(self, edges):
        n = len(edges[0])
        if self.n_edges + n > _sv.POSE_GRAPH_EDGES_MAX:
            raise ValueError("a pose graph holds at most 2^22 edges")
        if self.n_edges + n > self.capacity:
            self._allocate(min(_sv.POSE_GRAPH_EDGES_MAX, max(2 * self.capacity, self.n_edges + n)))
        for (name, _, _), a in zip(self._FIELDS, edges):
            self._host[name][self.n_edges:self.n_edges + n] = a
        self.n_edges += n

    def _send(self):
        import torch
        at = slice(self._sent, self.n_edges)
        for name in self._ON_DEVICE:
            getattr(self, name)[at] = torch.from_numpy(self._host[name][at]).to(self.device)
        self._sent = self.n_edges

    def add_chain(self, poses, w_rot=1.0, w_trans=1.0, fixed=(0,)):
        """The poses of the drive, float64 [N,12] world from frame (numpy: odometry's), and the odometry edges between neighbours with
        the weights given (scalars or [N - 1]); fixed: the poses held, indices or a bool mask.  Once per graph, before any loop."""
        if len(self.poses):
            raise ValueError("the graph has its chain already")
        g = _sv.pose_graph(poses, [_sv.pose_graph_chain(poses, w_rot, w_trans)], fixed)  # the checks
        self.poses, self.fixed = g["poses"], g["fixed"]
        self._add((g["i"], g["j"], g["Z"], g["w"], g["kind"]))

    def add_loop(self, i, j, Z, w_rot=1.0, w_trans=1.0):
        """A loop edge: frames i and j and the measured Z = P_i^-1 o P_j [12] - say stereo_vision.sv.pose_between(the key's pose, the
        pose VoxelMap.align arrived at for frame j) - with its weights.  ValueError for what stereo_vision.sv.pose_graph refuses of an
        edge, and before add_chain."""
        e = _sv.pose_graph_loop(i, j, Z, w_rot, w_trans)
        N = len(self.poses)
        if N == 0:
            raise ValueError("add_chain comes first")
        if not (0 <= e[0][0] < N and 0 <= e[1][0] < N) or e[0][0] == e[1][0]:
            raise ValueError("a loop ties two different frames in 0 .. %d, got %d and %d" % (N - 1, e[0][0], e[1][0]))
        if not np.isfinite(e[2]).all() or not np.isfinite(e[3]).all() or (e[3] < 0).any():
            raise ValueError("Z must be finite, the weights finite and not negative")
        self._add(e)

    def graph(self):
        """stereo_vision.sv.pose_graph's dict of the graph as it stands, on the host: views, checked when they were added."""
        n = self.n_edges
        return dict({"poses": self.poses, "fixed": self.fixed}, **{name: self._host[name][:n] for name, _, _ in self._FIELDS})

    def optimize(self, rounds=10, gate=None, eps=1e-9, lam=1e-6, max_iters=None, tol=1e-8):
        """stereo_vision.sv.pose_graph_optimize on the graph -> (the corrected poses float64 [N,12], numpy; the stats dict: costs, cost,
        iterations, converged, off, rounds).  max_iters caps PCG per round, None is max(1000, 20 N); a round that stops at the cap is an
        inexact step and shows as False in stats["converged"].  The poses of the chain stay what they were: corrections() holds the two
        against each other."""
        if not len(self.poses):
            raise ValueError("add_chain comes first")
        on = None
        if self.device.type == "cuda":
            self._send()
            on = {name: getattr(self, name)[:self.n_edges] for name in self._ON_DEVICE}
        self.optimized, stats = pose_graph_optimize(self.graph(), rounds, gate, eps, lam, max_iters, tol, device=self.device if on else None, device_edges=on, checked=True)
        return self.optimized, stats

    def corrections(self):
        """stereo_vision.sv.pose_corrections(the chain's poses, the optimised ones): float64 [N,12], what VoxelMap.repose and
        PlaceIndex.repose take."""
        if self.optimized is None:
            raise ValueError("optimize() has not run")
        return _sv.pose_corrections(self.poses, self.optimized)


class OccupancyMap:
    """A world-fixed occupancy map (include/stereo_vision_hip.h (K), stereo_vision.sv.occupancy_fuse): logodds int16 and last_seen int32
    [rows,cols] over x_range x y_range (metres, integer-valued bounds) at `scale` uniform cells per metre, and a spare pair of the same
    size for scrolling.  device: a CUDA device ("cuda", "cuda:1", an index) - engine.occupancy_fuse, one kernel per update - or "cpu" -
    the numpy definition on CPU tensors, the same methods and the same bits.  log_odds_words: l_occ, l_free, l_min, l_max (log-odds times
    100).  words is the map's sv_occupancy_map_spec as a dict (top and left move with recenter), seq the number of frames fused so far:
    the sequence number the next frame carries into last_seen.  clearance() and check_paths() are group (M): the squared distance to the nearest
    obstacle per cell, and candidate paths checked against it; clearance_radius is the radius in cells of the last clearance().
    cost_to_goal() and routes() are group (N): the length of the cheapest path from every cell to a goal, and the cells to drive.
    frontiers() and frontier_goals() are group (O): the free cells that touch undecided space, their clusters and one goal per cluster -
    the loop clearance -> cost_to_goal(any goal) or cost_cells -> frontiers -> cost_to_goal(frontier_goals) -> routes(vehicle).
    view() and frontier_views() are group (P): the distinct cells the vehicle would see from candidate poses, and with them a heading and a
    worth per frontier - frontiers -> frontier_views -> cost_to_goal(the goals worth the trip) -> routes.
    load_voxels() is group (V), stereo_vision.sv.voxel_map_flatten: the map's words replaced by a VoxelMap's evidence, sliced by height,
    so that the planner runs on the voxel map - vm.update -> vm.carve -> om.load_voxels(vm) -> clearance -> cost_to_goal -> routes."""

    def __init__(self, x_range, y_range, scale, device="cuda", **log_odds_words):
        import torch
        self.words = _sv.occupancy_map_params(x_range, y_range, scale, **log_odds_words)
        self.device = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:  # "cuda": the current device, named as its tensors name it
            self.device = torch.device("cuda", torch.cuda.current_device())
        shape = (self.words["rows"], self.words["cols"])
        self.logodds, self._spare_logodds = (torch.zeros(shape, dtype=torch.int16, device=self.device) for _ in range(2))
        self.last_seen, self._spare_last_seen = (torch.full(shape, -1, dtype=torch.int32, device=self.device) for _ in range(2))
        self.seq = 0
        self._d2, self._clearance_workspace, self.clearance_radius = None, None, None  # clearance()'s, made on its first call
        self._pen, self._cost, self._cost_workspace = None, None, None  # cost_to_goal()'s, made on its first call
        self._frontier_mask, self._frontiers = None, None  # frontiers()'s, made on its first call
        self._view = None  # view()'s result and workspace, made on its first call
        self._flatten = None  # load_voxels()'s result, made on its first call

    def reset(self):
        """A fresh map at the place it has scrolled to: logodds 0, last_seen -1, seq 0."""
        self.logodds.zero_()
        self.last_seen.fill_(-1)
        self.seq = 0

    def _fuse(self, state, poses, frame_grid, shift):
        """One fuse call from the map's pair into itself (no shift) or into the spare pair, which then becomes the map."""
        import torch
        moved = shift != (0, 0)
        going_out = dict(self.words, top=self.words["top"] - shift[0], left=self.words["left"] - shift[1])
        if self.device.type == "cuda":
            out = (self._spare_logodds, self._spare_last_seen) if moved else None
            occupancy_fuse(state, poses, frame_grid, going_out, self.logodds, self.last_seen, self.seq, shift, out=out)
        else:
            p = poses.cpu().numpy() if isinstance(poses, torch.Tensor) else poses
            res = _sv.occupancy_fuse(state.numpy(), p, frame_grid, going_out, self.logodds.numpy(), self.last_seen.numpy(), self.seq, shift)
            self._spare_logodds.copy_(torch.from_numpy(res["logodds"]))
            self._spare_last_seen.copy_(torch.from_numpy(res["last_seen"]))
            moved = True
        if moved:
            self.logodds, self._spare_logodds = self._spare_logodds, self.logodds
            self.last_seen, self._spare_last_seen = self._spare_last_seen, self.last_seen

    def update(self, states, poses, frame_grid=None):
        """Fuses B frames, in order: states uint8 [B,frame rows,frame cols] on the map's device with frame_grid (a dict of x_range,
        y_range, scale, or an engine.SvOccupancySpec), or an engine.OccupancyResult (StereoRig.occupancy's: its state and its spec);
        poses float64 [B,4] = (tx, ty, c, s) (stereo_vision.sv.occupancy_pose), numpy or a tensor.  Not waited for."""
        states, frame_grid = self._states(states, frame_grid, "update")
        self._fuse(states, poses, frame_grid, (0, 0))
        self.seq += states.shape[0]

    def _states(self, states, frame_grid, what):
        """update's first two arguments -> (uint8 tensor [B,frame rows,frame cols] on the map's device, frame grid)."""
        import torch
        if not isinstance(states, (torch.Tensor, np.ndarray)):
            states, frame_grid = states.state, states.spec if frame_grid is None else frame_grid
        if isinstance(states, np.ndarray):
            states = torch.from_numpy(states).to(self.device)
        if frame_grid is None:
            raise ValueError("%s: states given as a tensor need the frame_grid they were made under" % what)
        if not isinstance(states, torch.Tensor) or states.device != self.device or states.dtype != torch.uint8:
            raise ValueError("%s: states must be uint8 on %s" % (what, self.device))
        return (states.unsqueeze(0) if states.dim() == 2 else states), frame_grid

    def match(self, states, poses, frame_grid=None, w_occ=1, w_free=0):
        """Scores B frames against the map as it stands (stereo_vision.sv.occupancy_match): states as for update, poses float64 [B,P,4] =
        (tx, ty, c, s), numpy or a tensor - frame b's own P candidates.  -> engine.MapMatchResult with sums [B,P,2], counts [B,P,2], best
        [B] and best_score [B] as tensors on the map's device.  The map is not changed; not waited for."""
        import torch
        from .engine import MapMatchResult
        states, frame_grid = self._states(states, frame_grid, "match")
        if self.device.type == "cuda":
            return occupancy_match(states, poses, frame_grid, self.words, self.logodds, w_occ, w_free)
        p = poses.cpu().numpy() if isinstance(poses, torch.Tensor) else poses
        res = _sv.occupancy_match(states.numpy(), p, frame_grid, self.words, self.logodds.numpy(), w_occ, w_free)
        return MapMatchResult(**{k: torch.from_numpy(np.ascontiguousarray(res[k])) for k in MapMatchResult.__slots__})

    def localize(self, states, guess_xyyaw, half, steps, frame_grid=None, w_occ=1, w_free=0):
        """The best pose per frame of a window around its guess: guess_xyyaw float64 [B,3] = (x, y, yaw) ([3] for one frame), half = (dx,
        dy, dyaw) and steps = (nx, ny, nyaw) as stereo_vision.sv.occupancy_pose_window takes them - the guess is candidate 0 and keeps
        ties.  -> (float64 numpy [B,3], the refined (x, y, yaw); the MapMatchResult).  Waits for the best indices - B words - and reads
        nothing else back."""
        states, frame_grid = self._states(states, frame_grid, "localize")
        g = np.asarray(guess_xyyaw, np.float64)
        g = g[None] if g.ndim == 1 else g
        if g.shape != (states.shape[0], 3):
            raise ValueError("localize: guess_xyyaw must be [%d,3], got %s" % (states.shape[0], g.shape))
        window = np.stack([_sv.occupancy_pose_window(x, y, yaw, half, steps) for x, y, yaw in g]) if len(g) else np.zeros((0, 1, 3))
        res = self.match(states, _sv.occupancy_pose(window[..., 0], window[..., 1], window[..., 2]), frame_grid, w_occ, w_free)
        best = res.best.cpu().numpy().astype(np.int64)
        return window[np.arange(len(g)), best], res

    def recenter(self, x, y):
        """Scrolls the map by whole cells so that the world point (x, y) lies in its middle cell (rows // 2, cols // 2); what scrolls out
        is lost, what scrolls in is fresh.  -> (shift_rows, shift_cols), the cells it moved by."""
        import torch
        shift = _sv.occupancy_recenter_shift(self.words, x, y)
        if shift != (0, 0):
            empty = torch.empty((0, 2, 2), dtype=torch.uint8, device=self.device)
            self._fuse(empty, np.zeros((0, 4)), dict(x_range=(0, 1), y_range=(0, 1), scale=1), shift)
            self.words = dict(self.words, top=self.words["top"] - shift[0], left=self.words["left"] - shift[1])
        return shift

    def load_voxels(self, voxel_map, **flatten):
        """Replaces the map's logodds and last_seen by a VoxelMap's, flattened at the map's current top and left (VoxelMap.flatten, whose
        keywords - z_ref, step, height, radius, min_obstacle, min_ground, min_n, min_rows, since - are taken here): the evidence is the
        voxel map's, nothing of the map's own is blended in.  seq becomes one past the largest last_seen, 0 for an empty result, and the
        results of clearance(), cost_to_goal(), frontiers() and view() that the map holds are dropped:
        `om.load_voxels(vm); om.clearance(...); om.cost_to_goal(...)` is the idiom.  -> the engine.VoxelFlattenResult, whose logodds and
        last_seen are the map's own tensors; floor, top, cells and stats stay with the map and are written again by the next call.  Waits
        for one word, the largest last_seen."""
        from .engine import VoxelFlattenResult
        if not isinstance(voxel_map, VoxelMap) or voxel_map.device != self.device:
            raise ValueError("load_voxels: a VoxelMap on the map's device (%s) is needed" % (self.device,))
        if self.device.type == "cuda":
            old = self._flatten
            out = VoxelFlattenResult(logodds=self.logodds, last_seen=self.last_seen, **({} if old is None else {k: getattr(old, k) for k in ("floor", "top", "cells", "stats")}))
            res = voxel_map.flatten(self.words, out=out, **flatten)
        else:
            res = voxel_map.flatten(self.words, **flatten)
            self.logodds.copy_(res.logodds)
            self.last_seen.copy_(res.last_seen)
            res.logodds, res.last_seen = self.logodds, self.last_seen
        self._flatten = res
        self.seq = int(self.last_seen.max()) + 1  # -1 everywhere: 0
        self._d2, self.clearance_radius, self._pen, self._cost, self._frontier_mask, self._frontiers, self._view = None, None, None, None, None, None, None
        return res

    def clearance(self, radius_m, occupied=None, unknown=False):
        """The clearance field of the map as it stands (stereo_vision.sv.occupancy_clearance): uint16 [rows,cols] on the map's device, per
        cell the squared distance in cells to the nearest cell with logodds >= occupied (default l_occ, as state()) - and, with unknown,
        to the nearest cell never seen - 65535 beyond the radius of ceil(radius_m scale) cells (ValueError above 254).  The tensor and
        its workspace stay with the map and are written again by the next call; check_paths uses them.  Not waited for."""
        import torch
        if not np.isfinite(radius_m) or radius_m <= 0:
            raise ValueError("clearance: the radius must be a positive number of metres, got %r" % (radius_m,))
        R = int(np.ceil(float(radius_m) * self.words["scale"]))
        if not 1 <= R <= _sv.CLEARANCE_RADIUS_MAX:
            raise ValueError("clearance: %r m are %d cells at scale %d: 1 .. 254" % (radius_m, R, self.words["scale"]))
        t_occ = self.words["l_occ"] if occupied is None else occupied
        if self.device.type == "cuda":
            if self._d2 is None:
                self._d2 = torch.empty(self.logodds.shape, dtype=torch.uint16, device=self.device)
                self._clearance_workspace = torch.empty((self.logodds.numel() + 15) // 16 * 16, dtype=torch.uint8, device=self.device)
            occupancy_clearance(self.logodds, R, t_occ, self.last_seen, unknown, out=self._d2, workspace=self._clearance_workspace)
        else:
            self._d2 = torch.from_numpy(_sv.occupancy_clearance(self.logodds.numpy(), R, t_occ, self.last_seen.numpy(), unknown))
        self.clearance_radius = R
        return self._d2

    def check_paths(self, paths, discs_m, d2=None):
        """K candidate paths checked against the last clearance() (or the field d2 of the same radius): paths float64 [K,T,3] = (x, y,
        yaw) or [K,T,4] = (tx, ty, c, s) poses, numpy or a tensor; discs_m [n,3] = (px, py, radius) in metres in vehicle axes, the
        footprint (stereo_vision.sv.clearance_discs rounds the radii up to whole cells; none may exceed clearance()'s).
        -> engine.ClearancePathsResult with first_hit, min_d2 and n_outside as int32 tensors [K] on the map's device.  Not waited for."""
        import torch
        from .engine import ClearancePathsResult
        d2 = self._d2 if d2 is None else d2
        if d2 is None:
            raise ValueError("check_paths: no clearance field yet - call clearance() first")
        discs = _sv.clearance_discs(discs_m, self.words["scale"])
        p = paths
        if not isinstance(p, torch.Tensor):
            p = np.asarray(p, np.float64)
        if p.ndim != 3 or p.shape[2] not in (3, 4):
            raise ValueError("check_paths: paths must be [K,T,3] = (x, y, yaw) or [K,T,4] poses, got %s" % (tuple(p.shape),))
        if p.shape[2] == 3:
            p = p.cpu().numpy() if isinstance(p, torch.Tensor) else p
            p = _sv.occupancy_pose(p[..., 0], p[..., 1], p[..., 2])
        if self.device.type == "cuda":
            return clearance_paths(d2, self.words, p, discs, self.clearance_radius)
        p = p.cpu().numpy() if isinstance(p, torch.Tensor) else p
        res = _sv.clearance_paths(d2.numpy(), self.words, p, discs[0], discs[1], self.clearance_radius)
        return ClearancePathsResult(**{k: torch.from_numpy(res[k]) for k in ClearancePathsResult.__slots__})

    def cost_to_goal(self, goal_xy, block_m, soft_m=0.0, weight=0, max_sweeps=4096):
        """The cost-to-goal field of the map under the last clearance() (stereo_vision.sv.cost_cells and cost_to_goal): goal_xy float64
        [G,2] ([2] for one goal) world points in metres - stereo_vision.sv.occupancy_cells_of names their cells; a cell within block_m
        of an obstacle is blocked (r2_block = ceil(block_m scale)^2; ValueError if that radius exceeds clearance()'s), a free cell
        nearer than soft_m pays weight per cell of the difference (soft = ceil(soft_m scale)).  -> engine.CostToGoalResult with cost
        int32 [rows,cols] on the map's device, converged and sweeps; with converged == False (max_sweeps reached) the field is an upper
        bound of the definition.  pen, cost and the workspace stay with the map and are written again by the next call; routes() uses
        them.  Waits for 16 bytes per round of sweeps."""
        import torch
        from .engine import CostToGoalResult
        if self._d2 is None:
            raise ValueError("cost_to_goal: no clearance field yet - call clearance() first")
        for v, what in ((block_m, "block_m"), (soft_m, "soft_m")):
            if not np.isfinite(v) or v < 0:
                raise ValueError("cost_to_goal: %s must be a number of metres >= 0, got %r" % (what, v))
        block, soft = (int(np.ceil(float(v) * self.words["scale"])) for v in (block_m, soft_m))
        if block > self.clearance_radius:
            raise ValueError("cost_to_goal: block_m = %r m are %d cells, beyond the %d of the last clearance()" % (block_m, block, self.clearance_radius))
        g = np.asarray(goal_xy, np.float64)
        goals = _sv.occupancy_cells_of(self.words, g[None] if g.ndim == 1 else g)
        if self.device.type == "cuda":
            if self._pen is None:
                self._pen = torch.empty(self.logodds.shape, dtype=torch.uint8, device=self.device)
                self._cost = torch.empty(self.logodds.shape, dtype=torch.int32, device=self.device)
            cost_cells(self._d2, self.clearance_radius, block * block, soft, weight, out=self._pen)
            res = occupancy_cost_to_goal(self._pen, goals, max_sweeps=max_sweeps, out=self._cost, workspace=self._cost_workspace)
            self._cost_workspace = res.workspace
            return res
        pen = _sv.cost_cells(self._d2.numpy(), block * block, soft, weight, radius=self.clearance_radius)
        self._pen, self._cost = torch.from_numpy(pen), torch.from_numpy(_sv.cost_to_goal(pen, goals))
        return CostToGoalResult(cost=self._cost, converged=True, sweeps=None)

    def routes(self, start_xy, capacity=4096):
        """K routes down the last cost_to_goal() (stereo_vision.sv.cost_routes): start_xy float64 [K,2] ([2] for one) world points in
        metres.  -> (engine.CostRoutesResult with cells int16 [K,capacity,2], length and status int32 [K] on the map's device; xy float64
        numpy [K,capacity,2], the centres of the routes' cells as centres() gives them, NaN past a route's length).  Waits for the
        cells, which xy is made from."""
        import torch
        from .engine import CostRoutesResult
        if self._cost is None:
            raise ValueError("routes: no cost-to-goal field yet - call cost_to_goal() first")
        s = np.asarray(start_xy, np.float64)
        starts = _sv.occupancy_cells_of(self.words, s[None] if s.ndim == 1 else s)
        if self.device.type == "cuda":
            res = cost_routes(self._cost, self._pen, starts, capacity)
        else:
            got = _sv.cost_routes(self._cost.numpy(), self._pen.numpy(), starts, capacity)
            res = CostRoutesResult(**{k: torch.from_numpy(got[k]) for k in CostRoutesResult.__slots__})
        cells = res.cells.cpu().numpy().astype(np.int64)
        Xw, Yw = self.centres()
        on = cells[..., 0] >= 0
        xy = np.stack([np.where(on, Xw[np.where(on, cells[..., 0], 0)], np.nan), np.where(on, Yw[np.where(on, cells[..., 1], 0)], np.nan)], -1)
        return res, xy

    def frontiers(self, min_cells=8, capacity=1024, occupied=None, free=None, reachable=True):
        """The frontier clusters of the map as it stands (stereo_vision.sv.frontier_cells and frontier_clusters): the free cells that
        touch a cell nobody has decided yet, grouped into 8-connected clusters of at least min_cells cells, at most capacity of them in
        the order a scan of the map meets them.  occupied and free default as state()'s.  reachable: a cell that the pen of the last
        cost_to_goal() blocks is no frontier cell (ValueError if there is no cost_to_goal() yet); False: no pen.  -> engine.FrontierResult
        with label int32 [rows,cols], clusters int32 [capacity,8], sums int64 [capacity,2] and info int32 [4] on the map's device.  The
        tensors and the workspace stay with the map and are written again by the next call.  Not waited for.

        The exploration loop: clearance -> cost_to_goal(any goal) or cost_cells -> frontiers -> cost_to_goal(frontier_goals) ->
        routes(vehicle): the route from the vehicle's cell ends at the frontier that is cheapest to reach."""
        import torch
        from .engine import FrontierResult
        occupied = self.words["l_occ"] if occupied is None else occupied
        free = -self.words["l_free"] if free is None else free
        if reachable and self._pen is None:
            raise ValueError("frontiers: reachable needs the pen of a cost_to_goal() - call it first, or pass reachable=False")
        pen = self._pen if reachable else None
        if self.device.type == "cuda":
            if self._frontier_mask is None:
                self._frontier_mask = torch.empty(self.logodds.shape, dtype=torch.uint8, device=self.device)
            frontier_cells(self.logodds, self.last_seen, occupied, free, pen=pen, out=self._frontier_mask)
            old = self._frontiers
            reuse = old is not None and old.clusters.shape[0] == capacity
            self._frontiers = frontier_clusters(self._frontier_mask, min_cells, capacity, out=old if reuse else None, workspace=old.workspace if reuse else None)
            return self._frontiers
        self._frontier_mask = torch.from_numpy(_sv.frontier_cells(self.logodds.numpy(), self.last_seen.numpy(), occupied, free, None if pen is None else pen.numpy()))
        got = _sv.frontier_clusters(self._frontier_mask.numpy(), min_cells, capacity)
        self._frontiers = FrontierResult(**{k: torch.from_numpy(got[k]) for k in ("label", "clusters", "sums", "info")})
        return self._frontiers

    def frontier_goals(self, result=None):
        """The goals the clusters of a frontiers() result offer (the last one's where none is given): float64 numpy [n,2] = (Xw, Yw),
        the centres of the representatives of the written rows (stereo_vision.sv.frontier_goals) - what cost_to_goal takes, the next
        step of the loop clearance -> cost_to_goal(any goal) or cost_cells -> frontiers -> cost_to_goal(frontier_goals) ->
        routes(vehicle).  Waits for info and the written rows only."""
        result = self._frontiers if result is None else result
        if result is None:
            raise ValueError("frontier_goals: no frontiers yet - call frontiers() first")
        n = int(result.info.cpu().numpy()[3])
        return _sv.frontier_goals(self.words, result.clusters[:n].cpu().numpy())

    def view(self, poses, fov, range_m, n_rays=128, max_unknown=0, occupied=None, free=None):
        """What the vehicle would see of the map as it stands from candidate poses (stereo_vision.sv.occupancy_view): poses float64 [K,3]
        or [G,P,3] = (x, y, yaw), or [...,4] = (tx, ty, c, s), numpy or a tensor - [K,*] is K groups of one candidate; a fan of n_rays
        rays over fov radians that reach range_m metres (stereo_vision.sv.view_rays); max_unknown: the unknown cells a ray sees through
        (0: no limit); occupied and free default as state()'s.  -> engine.ViewResult with counts int32 [G,P,3] = (unknown, free,
        occupied) distinct cells seen, end_cells int16 [G,P,n_rays,2], status uint8 [G,P,n_rays], best and best_score int32 [G] on the
        map's device.  The tensors and the workspace stay with the map and are written again by the next call of the same shapes.  Not
        waited for."""
        import torch
        from .engine import ViewResult
        occupied = self.words["l_occ"] if occupied is None else occupied
        free = -self.words["l_free"] if free is None else free
        ends, reach = _sv.view_rays(fov, n_rays, range_m, self.words["scale"])
        p = poses
        if not isinstance(p, torch.Tensor):
            p = np.asarray(p, np.float64)
        if p.ndim not in (2, 3) or p.shape[-1] not in (3, 4):
            raise ValueError("view: poses must be [K,3] or [G,P,3] = (x, y, yaw), or [...,4] poses, got %s" % (tuple(p.shape),))
        if p.shape[-1] == 3:
            p = p.cpu().numpy() if isinstance(p, torch.Tensor) else p
            p = _sv.occupancy_pose(p[..., 0], p[..., 1], p[..., 2])
        if p.ndim == 2:
            p = p[:, None, :]
        if self.device.type == "cuda":
            old = self._view
            shape = (p.shape[0], p.shape[1], len(ends), 2)
            reuse = old is not None and tuple(old.end_cells.shape) == shape
            self._view = occupancy_view(self.logodds, self.last_seen, self.words, p, ends, reach, occupied, free, max_unknown, out=old if reuse else None,
                                        workspace=None if old is None else old.workspace)
            return self._view
        p = p.cpu().numpy() if isinstance(p, torch.Tensor) else p
        got = _sv.occupancy_view(self.logodds.numpy(), self.last_seen.numpy(), self.words, p, ends, reach, occupied, free, max_unknown)
        self._view = ViewResult(**{k: torch.from_numpy(np.ascontiguousarray(got[k])) for k in ("counts", "end_cells", "status", "best", "best_score")})
        return self._view

    def frontier_views(self, result=None, headings=16, fov=np.pi / 2, range_m=10.0, n_rays=128, max_unknown=0):
        """The best arrival pose per frontier: the goals of a frontiers() result (the last one's where none is given) crossed with
        `headings` yaws 2 pi p / headings (stereo_vision.sv.view_headings), each viewed as view() does; the best heading of a frontier
        is the first that sees the most unknown cells.  -> (float64 numpy [n,3] = (x, y, yaw), the ViewResult with counts [n,headings,3]).
        Waits for best and best_score only - 2 n words - beside what frontier_goals reads."""
        goals = self.frontier_goals(result)
        window = _sv.view_headings(goals, headings)  # [n, headings, 4]
        res = self.view(window, fov, range_m, n_rays, max_unknown)
        best = res.best.cpu().numpy().astype(np.int64)
        yaw = 2 * np.pi * np.arange(int(headings), dtype=np.float64) / int(headings)
        return np.stack([goals[:, 0], goals[:, 1], yaw[best]], 1), res

    def centres(self):
        """(Xw float64 [rows], Yw float64 [cols]) numpy: the world coordinates of the cells' centres."""
        return _sv.occupancy_map_centres(self.words)

    def state(self, occupied=None, free=None):
        """uint8 [rows,cols] on the map's device: 2 where logodds >= occupied (default l_occ: one occupied observation), else 1 where
        logodds <= free (default -l_free), in cells seen at least once (last_seen >= 0); else 0."""
        import torch
        occupied = self.words["l_occ"] if occupied is None else occupied
        free = -self.words["l_free"] if free is None else free
        L = self.logodds
        two, one, zero = (torch.full_like(L, v, dtype=torch.uint8) for v in (2, 1, 0))
        return torch.where(self.last_seen >= 0, torch.where(L >= occupied, two, torch.where(L <= free, one, zero)), zero)
