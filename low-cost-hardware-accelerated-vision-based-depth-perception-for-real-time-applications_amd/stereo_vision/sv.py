"""Counterpart of the reference's Python entry point (reference: stereo_vision/sv.py) over libstereo_vision_hip.so.

Same class, constructor arguments, ctypes signature and CLI flags as the reference:

    class stereo_vision(so_lib_path, width, height, defaultCalibFile, objectTracking, graphics, display, scale,
                        pc_extrapolation, YOLO_CFG, YOLO_WEIGHTS, YOLO_CLASSES, CAMERA_CALIBRATION_YAML, subsampling)
        .generatePointCloud(left_bgr, right_bgr) -> ndarray (width*height, 3) float64      (sv.py:156-189)
    main()  argparse CLI                                                                    (sv.py:195-331)

Differences, all forced by the environment or by bugs of the reference:
  * no cv2: BGR->BGRA is a numpy concatenate, images are read with PIL;
  * the C function is called with the reference's 14 arguments (sv.py:180,189); the library does not read arguments 15/16
    (removeSky, subsampling) - half-resolution mode is selected with sv_legacy_set_subsampling() before the first frame;
  * __del__ calls clean(), which here frees the library state but does NOT exit() the interpreter;
  * the dataset download helpers of the reference's CLI are not provided (no network); --demo reads --kitti.

The reference's top-view helpers (sv.py:87-134) are here as a numpy restatement with the same names and signatures:
normalize_depth, in_range_points and points_2_top_view (plus mode="count").  They are the CPU form of engine.top_view /
engine.top_view_from_disparity / rig.StereoRig.top_view and the tests' oracle.  Deviations: a value whose
quotient is negative (dist > max_dist) is 0; non-integer x / y ranges, lo >= hi, a scale that is not a positive integer and
max_dist == 0 in "reference" mode raise ValueError.

box_positions is the numpy restatement of the batched object positions (sv_box_positions_* of include/stereo_vision_hip.h (E);
engine.box_positions / engine.box_positions_from_disparity / rig.StereoRig.box_positions on the GPU): the mean point inside each
detector box in the library's summation order, usable without a GPU and the tests' oracle.  stereo_vision.object_positions stays
the reference's one-frame form.

compact_cloud is the numpy restatement of the compact coloured point clouds (sv_cloud_* of include/stereo_vision_hip.h (F);
engine.compact_cloud_from_disparity / rig.StereoRig.compact_clouds on the GPU): per frame the valid, cropped, thinned-out points in
pixel order with their colours and pixel indices - the pairing of points[i] with colors[i] the reference's viewer draws
(src/common_includes/graphing.h:123-133).  write_ply stores one as a binary PLY file.

voxel_cloud is the definition of the voxel-grid downsampled clouds (sv_voxel_* of include/stereo_vision_hip.h (I);
engine.voxel_cloud_from_disparity / rig.StereoRig.voxel_clouds on the GPU): compact_cloud's points gathered per cell of a regular 3-D
grid - centroid, mean colour, number of points - with integer sums only, so that the result does not depend on any order.  The reference
has no counterpart.

v_disparity, ground_line, ground_labels, free_space (together: ground), ground_pose and free_space_points are the definition of the ground
plane, obstacle labels and free space (sv_ground_* of include/stereo_vision_hip.h (G); engine.ground_from_disparity /
rig.StereoRig.ground on the GPU): Labayrade's v-disparity line fit in integers and a per-column scan for the nearest obstacle.  The
reference has no counterpart.

occupancy_params, occupancy_grid (with occupancy_ray_cells / occupancy_ray_clip) and occupancy_heights are the definition of the
occupancy and elevation grids (sv_occupancy_* of include/stereo_vision_hip.h (J); engine.occupancy_from_disparity /
rig.StereoRig.occupancy on the GPU): per cell of the top view's grid the ground and obstacle pixels that fell into it, the height span
of what was seen, the sight lines that crossed it and a state - unknown, free or occupied.  Integers from the cell index on.  The
reference has no counterpart.

occupancy_map_params, occupancy_pose and occupancy_fuse (with occupancy_map_words, occupancy_map_centres, occupancy_scroll,
occupancy_recenter_shift and occupancy_map_state) are the definition of the world-fixed occupancy map (the fuse entry of
include/stereo_vision_hip.h (K); engine.occupancy_fuse / rig.OccupancyMap on the GPU): the states of the frames of a drive fused along
the poses of its odometry into one log-odds map of uniform cells that accumulates evidence, comes back down where a cell is seen free
again, and scrolls by whole cells with the vehicle.  Doubles in a stated order up to the cell index, integers behind it.  The reference
has no counterpart.

occupancy_match and occupancy_pose_window are the definition of the correlative match (sv_map_match_* of include/stereo_vision_hip.h (L);
engine.occupancy_match / rig.OccupancyMap.match and .localize on the GPU): a frame's occupied (and free) cells carried into the map at
every pose of a window around the odometry's guess, the map's log-odds summed under them, and the best pose named - so that a drifting
pose can be corrected before the frame is fused.  Integer sums behind the cell index: bit for bit.  The reference has no counterpart
(DESIGN.md §8).

occupancy_clearance (with occupancy_clearance_brute, the all-pairs form), clearance_paths and clearance_discs are the definition of the
clearance field and the path check (sv_clearance_* of include/stereo_vision_hip.h (M); engine.occupancy_clearance / engine.clearance_paths /
rig.OccupancyMap.clearance and .check_paths on the GPU): per map cell the squared distance in cells to the nearest occupied (or never seen)
cell, capped at a radius, and per candidate path the first step at which a footprint of discs touches an obstacle, the least clearance met
and the lookups that left the map.  Minima and counts of integers: bit for bit.  The reference has no counterpart.

cost_cells, cost_to_goal (with cost_to_goal_relax, the whole-array relaxation), cost_routes and occupancy_cells_of are the definition of
the cost-to-goal field and the routes traced through it (sv_cost_* of include/stereo_vision_hip.h (N); engine.cost_cells /
engine.occupancy_cost_to_goal / engine.cost_routes / rig.OccupancyMap.cost_to_goal and .routes on the GPU): per map cell a penalty made
from the clearance field, the length of the cheapest 8-connected path to the nearest goal that cuts no corner, and per start cell the
route that follows the field downhill.  Shortest paths under strictly positive integer weights: unique, so bit for bit.  The reference
has no counterpart.

frontier_cells, frontier_clusters (with frontier_labels, the union-find on its own) and frontier_goals are the definition of the frontiers
of the world map (sv_frontier_* of include/stereo_vision_hip.h (O); engine.frontier_cells / engine.frontier_clusters /
rig.OccupancyMap.frontiers and .frontier_goals on the GPU): the free cells that touch undecided space, their 8-connected clusters - label,
size, bounding box and a representative cell each, in the order a scan meets them - and the world points cost_to_goal takes as goals.
Labels are least indices and the statistics sums, minima and maxima of integers: bit for bit.  The reference has no counterpart
(DESIGN.md §8).

view_rays, view_headings, occupancy_view, view_ranges and view_lines are the definition of the expected view of the world map from
candidate poses (sv_view_* of include/stereo_vision_hip.h (P); engine.occupancy_view / rig.OccupancyMap.view and .frontier_views on the
GPU): rays cast through the map from each pose, the distinct cells they see counted by state - the unknown ones are what a trip there
would uncover -, the last visible cell of every ray - a virtual range scan - and the best pose per group.  The trigonometry stays on
the host; the walk is integers: bit for bit.  The reference has no counterpart.

voxel_map_params, voxel_map_pose, voxel_map_state, voxel_map_insert, voxel_map_rows and voxel_map_slot_of are the definition of the
world-fixed voxel map (sv_voxel_map_* of include/stereo_vision_hip.h (Q); engine.voxel_map_insert / voxel_map_rows and rig.VoxelMap on the
GPU): voxel_cloud's or compact_cloud's rows of the frames of a drive, moved into the world by one pose per frame and accumulated per cubic
cell - integer sums of weights, offsets and colours, the rows, the first and the last frame -, read out as one row per voxel in ascending
key.  The reference shows its cloud frame by frame and keeps none.

voxel_map_pose_window and voxel_map_match are the definition of a frame matched against the voxel map (sv_voxel_match_* of
include/stereo_vision_hip.h (R); engine.voxel_map_match / rig.VoxelMap.match and .localize on the GPU): the rows of a frame under every
pose of a window in x, y, z and yaw, looked up in the map - the rows that land in a voxel, their weight and their squared sub-cell
distance to the voxels' means per candidate, and the best candidate per frame -, so that a pose is corrected before the frame is
inserted.  The reference has no counterpart.

voxel_map_carry (with voxel_map_shifted and voxel_map_recenter_shift) is the definition of a voxel map carried into another
(sv_voxel_map_carry_device of include/stereo_vision_hip.h (S); engine.voxel_map_carry / rig.VoxelMap.prune, .recenter, .resize and .merge
on the GPU): the voxels of a map, filtered by weight, rows and age and shifted by whole cells, added into a second map - so that the map
scrolls with the vehicle, forgets, grows and takes in another map's voxels without leaving its integers.  The reference has no counterpart
(DESIGN.md §8).

voxel_map_carve is the definition of a voxel map carved by the sight lines of frames (sv_voxel_carve_device of
include/stereo_vision_hip.h (T); engine.voxel_map_carve / rig.VoxelMap.carve on the GPU): a ray per kept row from the sensor's cell to the
row's, occupancy_ray_cells' line rule on three axes, the weight of the rays that pass through a voxel no later frame has seen, and the
voxels emptied that enough of it passed through - so that the map un-sees what is no longer there.  The reference has no counterpart
(DESIGN.md §8).

voxel_map_render (with voxel_map_render_brute, the plain loop, voxel_render_camera and voxel_render_cams) is the definition of the voxel
map rendered into a camera (sv_voxel_render_device of include/stereo_vision_hip.h (U); engine.voxel_map_render / rig.VoxelMap.render on
the GPU): per view the nearest voxel under every pixel - its depth, key and colour -, the disparity the rig would measure there, and its
comparison with the disparity it did measure, pixel by pixel: nearer means something new, farther a voxel that was seen through.  The
3-D counterpart of occupancy_view.  The reference has no counterpart.

voxel_map_flatten (with voxel_map_flatten_brute, the plain loops, voxel_flatten_params and voxel_flatten_words) is the definition of the
voxel map flattened into an occupancy map (sv_voxel_flatten_device of include/stereo_vision_hip.h (V); engine.voxel_map_flatten /
rig.VoxelMap.flatten / rig.OccupancyMap.load_voxels on the GPU): the voxels sliced by their height above an absolute or a local floor into
ground, obstacle and overhead, and per flat cell the log-odds and last_seen words that occupancy_clearance, cost_to_goal, frontier_cells
and occupancy_view take - a bridge overhead is no obstacle, a kerb below the step is ground.  The reference has no counterpart (DESIGN.md
§8).

voxel_map_clusters (with voxel_map_clusters_brute, the plain flood fill, voxel_cluster_params, voxel_cluster_words and voxel_cluster_boxes)
is the definition of the voxel map clustered (sv_voxel_clusters_device of include/stereo_vision_hip.h (W); engine.voxel_map_clusters /
rig.VoxelMap.clusters / .despeckle on the GPU): the 6-, 18- or 26-connected components of the voxels inside a height band over an
absolute floor or over the flatten's, a row of counts, sums and a box per component in ascending least key, a label per voxel, and the
components below a size emptied - the objects of the map and its speckle filter in three dimensions.  The reference has no counterpart
(DESIGN.md §8).

voxel_map_align_sums (with voxel_map_align_sums_brute, the plain loop per row) is the definition of a frame aligned to the voxel map
(sv_voxel_align_* of include/stereo_vision_hip.h (X); engine.voxel_map_align_sums / voxel_map_align and rig.VoxelMap.align on the GPU):
every row of a frame paired with the nearest voxel mean of the map, and the pairs reduced to the nineteen integers a closed-form rigid
fit needs.  voxel_align_origin, voxel_align_solve and voxel_map_align are the host's part of iterative closest point - the origin the
sums are taken about, the fit (Kabsch for six degrees of freedom, about z alone for four) and the loop -, shared by the CPU and the GPU
path, so that both give the same poses bit for bit.  It refines a pose below voxel_map_match's step, and in roll and pitch.  The
reference has no counterpart.

voxel_map_normals (with voxel_map_normals_brute, the plain loop per voxel in Python ints and fractions, voxel_normal_dirs and
voxel_normal_vectors) is the definition of the voxels' surface normals (sv_voxel_normals_device of include/stereo_vision_hip.h (Y);
engine.voxel_map_normals / rig.VoxelMap.normals on the GPU): per voxel the plane through the means of the voxels around it, as the best
of a fixed table of integer directions under an exact integer criterion.  voxel_map_align_plane_sums (with
voxel_map_align_plane_sums_brute) is the definition of one round of point-to-plane alignment against them (sv_voxel_plane_align_*;
engine.voxel_map_align_plane_sums): voxel_map_align_sums' pairs, reduced to the 32 integers of the normal equations.
voxel_align_solve_plane is the host's fit, and voxel_map_align(method="plane") the loop around both - a row may slide along the plane it
lies on, so the loop needs a few rounds on a street where the point-to-point loop creeps.  The reference has no counterpart (DESIGN.md
§8).

flow_match and flow_pose_sums (with flow_pose_sums_brute, the plain loop per match in Python integers) are the definition of the stereo
visual odometry (sv_flow_* of include/stereo_vision_hip.h (Z); engine.flow_match / flow_pose_sums / flow_egomotion and
rig.StereoRig.flow / .odometry on the GPU): the lattice points of frame k - 1 that carry a disparity, found again in frame k by a sum of
absolute differences over a window around where a guessed motion puts them, and the matches reduced under a pose to the 32 integers of a
gated Gauss-Newton round.  flow_solve, flow_egomotion, flow_chain and flow_odometry are the fit, the loop, the chain of poses and the
drive, shared by the CPU and the GPU path, so that both give the same poses bit for bit.  Header comment of the details the issue left
open: FLOW_Z_MIN = 0.1 m; b = 1 / q32 with q33 taken as 0; a disparity makes a point where floor(16 d + 0.5) is in 1 .. 2^20; a window
centre beyond +-2^20 drops the point; rows behind a frame's count hold -1; a match is inside where z > z_min and its predicted words stay
within +-2^30; no gate is 2^20 sixteenths of a pixel; FLOW_EPS = (2e-5 rad, 2e-4 m).  The reference has no counterpart.

voxel_map_repose (with voxel_map_repose_brute, the plain loop per voxel) is the definition of a voxel map re-posed after a loop closure
(sv_voxel_repose_device of include/stereo_vision_hip.h (AD); engine.voxel_map_repose / rig.VoxelMap.repose and .merge(pose=...) on the
GPU): every voxel moved by the rigid correction of the frame that saw it last and accumulated into a second map, in the insert's
integers.  pose_corrections, loop_spread (with pose_log and pose_exp) and pose_repose are the host's helpers in doubles, shared by the
CPU and the GPU path: the corrections between two sets of poses, one loop's error spread along the chain, and the stored poses of a
PlaceIndex under the same corrections.  The reference has no counterpart.

pose_graph_linearize and pose_graph_pcg (with their *_brute twins, plain loops in Python floats) and pose_graph_sum are the definition
of the pose graph of confirmed loops (sv_pose_graph_* of include/stereo_vision_hip.h (AE); engine.pose_graph_linearize /
pose_graph_solve / pose_graph_optimize and rig.PoseGraph on the GPU): a trig-free residual per edge, the linearisation about a right
perturbation that needs only M = P_j^-1 o P_i per edge, a matrix-free H in two passes, a block-Jacobi preconditioner factored as L D
L^T, and conjugate gradients whose dot products follow one stated tree.  pose_graph, pose_graph_chain, pose_graph_loop and pose_between
build a checked graph; pose_graph_optimize is the loop of Gauss-Newton rounds with the gate on loop edges, host code shared by the CPU
and the GPU path, so that both give the same poses bit for bit.  The reference has no counterpart.
"""
import argparse
import ctypes
import glob
import os

import numpy as np
from numpy.ctypeslib import ndpointer

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_STEREO_VISION_SO_PATH = os.path.join(os.path.dirname(HERE), "libstereo_vision_hip.so")
DEFAULT_CALIBRATION = os.path.join(HERE, "data", "kitti_2011_09_26.yml")


# --top-view: the camera's (right, down, forward) to the helper's lidar axes (forward, left, up), and the grid the CLI writes
CAMERA_TO_VEHICLE = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
CLI_TOP_VIEW = {"x_range": (0, 40), "y_range": (-20, 20), "z_range": (-1.4, 1.0), "scale": 10}
TOP_VIEW_MODES = ("reference", "count")
# --ply: the crop of CLI_TOP_VIEW as (lo, hi) of a compact cloud
CLI_CLOUD_CROP = tuple(tuple(float(CLI_TOP_VIEW[k][i]) for k in ("x_range", "y_range", "z_range")) for i in (0, 1))


def _integer(v, what):
    f = float(v)
    if not (np.isfinite(f) and f == np.trunc(f)):
        raise ValueError("%s must be integer-valued, got %r" % (what, v))
    return f


def top_view_grid(x_range, y_range, z_range, scale, mode="reference"):
    """(rows, cols) of the top view, after the checks sv_top_view_dims makes (ValueError for a bad argument): x / y bounds
    integer-valued with |bound| <= 2^31, lo < hi for all three ranges, scale a positive integer, rows and cols <= 32768, and
    max_dist = sqrt(x1^2 + y1^2) > 0 in "reference" mode."""
    if mode not in TOP_VIEW_MODES:
        raise ValueError("mode must be one of %s, got %r" % (TOP_VIEW_MODES, mode))
    if isinstance(scale, bool) or not _integer(scale, "scale") >= 1:
        raise ValueError("scale must be a positive integer, got %r" % (scale,))
    s = int(scale)
    (x0, x1), (y0, y1) = [(_integer(r[0], name), _integer(r[1], name)) for r, name in ((x_range, "x_range"), (y_range, "y_range"))]
    z0, z1 = float(z_range[0]), float(z_range[1])
    for lo, hi, name in ((x0, x1, "x_range"), (y0, y1, "y_range"), (z0, z1, "z_range")):
        if not lo < hi:
            raise ValueError("%s needs lo < hi, got (%r, %r)" % (name, lo, hi))
    if max(abs(x0), abs(x1), abs(y0), abs(y1)) > 2.0 ** 31:
        raise ValueError("x / y bounds must lie within +-2^31")
    rows, cols = (x1 - x0) * s + 1, (y1 - y0) * s + 1
    if rows > 32768 or cols > 32768:
        raise ValueError("grid of %d x %d cells: at most 32768 in either dimension" % (rows, cols))
    if mode == "reference" and x1 == 0 and y1 == 0:
        raise ValueError("max_dist = sqrt(x1^2 + y1^2) is 0: no value can be normalised")
    return int(rows), int(cols)


def normalize_depth(val, min_v, max_v):
    """(uint8) trunc(((max_v - val) / (max_v - min_v)) * 255): near points get high values, like the driver's disparity image
    (the reference's sv.py:87-92).  A negative quotient (val > max_v) gives 0; the reference's cast of it is undefined."""
    q = ((max_v - val) / (max_v - min_v)) * 255
    return np.where(q > 0, q, 0).astype(np.uint8)


def in_range_points(points, x, y, z, x_range, y_range, z_range):
    """The entries of `points` whose (x, y, z) lie strictly inside the three ranges (NaN and +-inf never do)."""
    return points[np.logical_and.reduce((x > x_range[0], x < x_range[1], y > y_range[0], y < y_range[1], z > z_range[0], z < z_range[1]))]


def points_2_top_view(points, x_range, y_range, z_range, scale, mode="reference"):
    """Top view of one cloud `points` [N, >=3] (X forward, Y left, Z up; float64): a grid of rows = (x1 - x0) * scale + 1 by
    cols = (y1 - y0) * scale + 1 cells, point (X, Y) in cell (trunc(x1 s) - trunc(X s), trunc(y1 s) - trunc(Y s)).
    mode "reference": uint8, each cell the normalize_depth value of dist = sqrt(X^2 + Y^2) against max_dist = sqrt(x1^2 + y1^2) of
    the in-range point with the largest index (what the reference's img[y_img, x_img] = dist_lim leaves), 0 where empty.
    mode "count": int32, the number of in-range points per cell."""
    rows, cols = top_view_grid(x_range, y_range, z_range, scale, mode)
    s = float(int(scale))
    x1, y1 = float(x_range[1]), float(y_range[1])
    pts = np.asarray(points, dtype=np.float64)
    pts = pts.reshape(-1, pts.shape[-1])
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    idx = in_range_points(np.arange(len(pts)), x, y, z, x_range, y_range, z_range)
    X, Y = x[idx], y[idx]
    row = (np.trunc(x1 * s) - np.trunc(X * s)).astype(np.int64)
    col = (np.trunc(y1 * s) - np.trunc(Y * s)).astype(np.int64)
    # x0 s <= fl(X s) <= x1 s for x0 < X < x1 (monotone rounding, exact integer bounds), so 0 <= row <= (x1 - x0) s; y alike
    assert row.size == 0 or (row.min() >= 0 and row.max() < rows and col.min() >= 0 and col.max() < cols)
    flat = row * cols + col
    if mode == "count":
        return np.bincount(flat, minlength=rows * cols).astype(np.int32).reshape(rows, cols)
    max_dist = np.sqrt(x1 * x1 + y1 * y1)
    value = normalize_depth(np.sqrt(X * X + Y * Y), 0, max_dist)
    img = np.zeros(rows * cols, np.uint8)
    # the last (largest-index) point of each cell: the first occurrence in the reversed order
    cells, first = np.unique(flat[::-1], return_index=True)
    img[cells] = value[::-1][first]
    return img.reshape(rows, cols)


BOX_SELECT = {"all": 0, "valid": 1, "near": 2}
BOX_DISPARITY = {"dmap": 0, "d1": 1}
BOX_BINS = 4096


def box_bounds(box, width, height):
    """(i_lb, i_ub, j_lb, j_ub) of a box (x, y, w, h): columns [clamp(x), clamp(x + w)), rows [clamp(y), clamp(y + h)) with
    clamp(a) = min(max(a, 0), size - 1) - the reference's clamp (stereo_vision.cpp:263-264): the last column and row never belong
    to a box.  Python integers: x + w cannot overflow."""
    x, y, w, h = (int(v) for v in box)
    cl = lambda a, size: min(max(a, 0), size - 1)  # noqa: E731
    return cl(x, width), cl(x + w, width), cl(y, height), cl(y + h, height)


def box_quantise(disp, disparity="dmap"):
    """(q int32, valid bool, d float64) per pixel of a float32 map: "dmap": q = saturate_u8(round_half_even(4 d)) (NaN gives 0),
    valid = q > 0, d = q; "d1": q = min(round_half_even(4 d), 4095) where valid = d > 0 (0 elsewhere), d = the float itself."""
    if disparity not in BOX_DISPARITY:
        raise ValueError("disparity must be one of %s, got %r" % (sorted(BOX_DISPARITY), disparity))
    d = np.asarray(disp, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(d * np.float32(4.0))
        if disparity == "dmap":
            q = np.clip(np.where(np.isnan(r), np.float32(0), r), 0, 255).astype(np.int32)
            return q, q > 0, q.astype(np.float64)
        valid = d > 0
        q = np.where(valid, np.minimum(r, np.float32(BOX_BINS - 1)), np.float32(0)).astype(np.int32)
        return q, valid, d.astype(np.float64)


def _box_points(d, Q, XR, XT):
    """reproject()'s arithmetic on a [H,W] float64 disparity: [H,W,3] points (products and sums rounded one by one, as written)."""
    H, W = d.shape
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    jj, ii = np.mgrid[0:H, 0:W]
    x, y = ii.astype(np.float64), jj.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pos = [((Q[r, 0] * x + Q[r, 1] * y) + Q[r, 2] * d) + Q[r, 3] for r in range(4)]
        X, Y, Z = pos[0] / pos[3], pos[1] / pos[3], pos[2] / pos[3]
        if XR is not None or XT is not None:
            XR = np.eye(3) if XR is None else np.asarray(XR, np.float64).reshape(3, 3)
            XT = np.zeros(3) if XT is None else np.asarray(XT, np.float64).reshape(3)
            X, Y, Z = [((XR[r, 0] * X + XR[r, 1] * Y) + XR[r, 2] * Z) + XT[r] for r in range(3)]
    return np.stack([X, Y, Z], -1)


def _box_sum(P, sel):
    """The library's order on the box's points P [rows, cols, 3] (sel [rows, cols] bool or None = all): per column the selected
    points in ascending row order onto +0.0 - an explicit loop over the rows, the columns side by side -, then the column sums
    left to right onto +0.0 - an explicit loop over the columns."""
    rows, cols = P.shape[:2]
    col = np.zeros((cols, 3), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(rows):
            col = col + P[j] if sel is None else np.where(sel[j][:, None], col + P[j], col)
        acc = np.zeros(3, np.float64)
        for i in range(cols):
            acc = acc + col[i]
    return acc


def box_positions(points_or_disp, boxes, n_boxes=None, Q=None, XR=None, XT=None, select="all", disparity="dmap", band=4):
    """3-D position per detector box, the definition of include/stereo_vision_hip.h (E) in numpy.

    Q None: points_or_disp is an f64 cloud [H,W,3] (or [B,H,W,3]); only select="all".  Q given: a float32 disparity map [H,W] (or
    [B,H,W]), reprojected with Q (and XR / XT) as engine.reproject does - disparity "dmap": the driver's saturate(round(4 d)),
    "d1": the float itself, in metres.  boxes: int [M,4] (or [B,M,4]) = (x, y, w, h); n_boxes: boxes in use per frame (None = all).
    select "all" (the reference's mean: inf / NaN propagate), "valid" (valid pixels) or "near" (valid pixels within `band` quarter
    pixels of the box's lower-median quantised disparity).
    Returns (pos float64 [M,3], stat int32 [M,4] = (n_pixels, n_valid, q_med, n_selected)), with a leading B for batched input;
    rows at and beyond n_boxes are NaN / -1.  pos = sum / n_selected in the order of _box_sum (0 selected: NaN)."""
    if select not in BOX_SELECT:
        raise ValueError("select must be one of %s, got %r" % (sorted(BOX_SELECT), select))
    if disparity not in BOX_DISPARITY:
        raise ValueError("disparity must be one of %s, got %r" % (sorted(BOX_DISPARITY), disparity))
    if isinstance(band, bool) or int(band) != band or band < 0:
        raise ValueError("band must be an integer >= 0, got %r" % (band,))
    src = np.asarray(points_or_disp)
    from_points = Q is None
    if from_points and select != "all":
        raise ValueError("a point cloud has no disparity: only select=\"all\" applies")
    frame_dim = 3 if from_points else 2
    if src.ndim not in (frame_dim, frame_dim + 1) or (from_points and src.shape[-1] != 3):
        raise ValueError("expected %s, got shape %s" % ("points [B,H,W,3]" if from_points else "disp [B,H,W]", src.shape))
    batched = src.ndim == frame_dim + 1
    if not batched:
        src = src[None]
    bx = np.asarray(boxes)
    if bx.ndim == 2:
        bx = np.broadcast_to(bx[None], (src.shape[0],) + bx.shape)
    if bx.ndim != 3 or bx.shape[0] != src.shape[0] or bx.shape[2] != 4:
        raise ValueError("boxes must be [B,M,4] (or [M,4]), got shape %s" % (bx.shape,))
    B, M = bx.shape[:2]
    H, W = src.shape[1:3]
    nb = np.full(B, M) if n_boxes is None else np.clip(np.asarray(n_boxes).reshape(B), 0, M)
    pos = np.full((B, M, 3), np.nan)
    stat = np.full((B, M, 4), -1, np.int32)
    for b in range(B):
        if from_points:
            P = np.asarray(src[b], np.float64)
            q = valid = None
        else:
            q, valid, d = box_quantise(src[b], disparity)
            P = _box_points(d, Q, XR, XT)
        for m in range(int(nb[b])):
            i_lb, i_ub, j_lb, j_ub = box_bounds(bx[b, m], W, H)
            ncols, nrows = max(i_ub - i_lb, 0), max(j_ub - j_lb, 0)
            n_pixels = ncols * nrows
            win = (slice(j_lb, j_lb + nrows), slice(i_lb, i_lb + ncols)) if n_pixels else (slice(0, 0), slice(0, 0))
            n_valid = q_med = -1
            n_sel, sel = n_pixels, None
            if not from_points:
                qb, vb = q[win], valid[win]
                hist = np.bincount(qb[vb], minlength=BOX_BINS)
                n_valid = int(hist.sum())
                if n_valid:
                    q_med = int(np.searchsorted(np.cumsum(hist), (n_valid + 1) // 2))  # the first bin whose cumulative count reaches it
                if select == "valid":
                    sel, n_sel = vb, n_valid
                elif select == "near":
                    sel = vb & (np.abs(qb - q_med) <= int(band))
                    n_sel = int(sel.sum())
            total = _box_sum(P[win], sel)
            with np.errstate(divide="ignore", invalid="ignore"):
                pos[b, m] = total / np.float64(n_sel)
            stat[b, m] = (n_pixels, n_valid, q_med, n_sel)
    return (pos, stat) if batched else (pos[0], stat[0])


CLOUD_DISPARITY = {"dmap": 0, "d1": 1}
CLOUD_DTYPES = {"f32": 0, "f64": 1}


def cloud_crop(lo=None, hi=None, step=1, disparity="d1", dtype="f32"):
    """(lo float64 [3], hi float64 [3]) of a compact-cloud request after the checks sv_cloud_disparity_device makes (ValueError for a bad
    argument): None = every axis open, lo < hi per axis (NaN refused), step an integer in 1 .. 2^31 - 1, disparity / dtype known."""
    if disparity not in CLOUD_DISPARITY:
        raise ValueError("disparity must be one of %s, got %r" % (sorted(CLOUD_DISPARITY), disparity))
    if dtype not in CLOUD_DTYPES:
        raise ValueError("dtype must be one of %s, got %r" % (sorted(CLOUD_DTYPES), dtype))
    if isinstance(step, bool) or int(step) != step or not 1 <= step < 2 ** 31:
        raise ValueError("step must be an integer >= 1, got %r" % (step,))
    lo = np.full(3, -np.inf) if lo is None else np.array(lo, np.float64).reshape(-1)
    hi = np.full(3, np.inf) if hi is None else np.array(hi, np.float64).reshape(-1)
    if lo.shape != (3,) or hi.shape != (3,) or not (lo < hi).all():
        raise ValueError("the crop needs three lo < hi, got %r / %r" % (lo.tolist(), hi.tolist()))
    return lo, hi


def compact_cloud(disp, Q, XR=None, XT=None, lo=None, hi=None, step=1, disparity="d1", dtype="f32", colors=None):
    """Compact coloured point cloud(s), the definition of include/stereo_vision_hip.h (F) in numpy.

    disp: a float32 disparity map [H,W] (or [B,H,W]).  The pixels with x % step == 0 and y % step == 0 are visited in ascending flat
    index y * W + x; a candidate ("dmap": q = saturate_u8(round_half_even(4 d)) > 0, its point that of (double)q, the driver's cloud at a
    quarter of metric depth; "d1": d > 0, its point that of d itself, metres) is kept iff lo[k] < P[k] < hi[k] on all three axes of
    P = reproject(x, y, .) (then XR P + XT) - strictly, so inf and NaN never pass; None leaves lo / hi open.
    Returns (xyz [N,3] float32 - P.astype(float32), round to nearest even - or float64, color uint8 [N,4] = colors[y, x] (None without
    colors [H,W,4]), index int32 [N] = y * W + x); for batched input a list of such tuples, one per frame."""
    lo, hi = cloud_crop(lo, hi, step, disparity, dtype)
    d = np.asarray(disp, dtype=np.float32)
    if d.ndim not in (2, 3):
        raise ValueError("expected disp [H,W] or [B,H,W], got shape %s" % (d.shape,))
    batched = d.ndim == 3
    if not batched:
        d = d[None]
    B, H, W = d.shape
    col = None
    if colors is not None:
        col = np.asarray(colors)
        col = col[None] if col.ndim == 3 else col
        if col.dtype != np.uint8 or col.shape != (B, H, W, 4):
            raise ValueError("colors must be uint8 [B,H,W,4] matching disp, got %s %s" % (col.dtype, col.shape))
    s = int(step)
    flat = (np.arange(0, H, s)[:, None] * W + np.arange(0, W, s)[None]).astype(np.int32)  # the visited pixels, in order
    out = []
    for b in range(B):
        _, cand, dd = box_quantise(d[b], disparity)
        P = _box_points(dd, Q, XR, XT)[::s, ::s]
        keep = cand[::s, ::s].copy()
        with np.errstate(invalid="ignore"):
            for k in range(3):
                keep &= (lo[k] < P[..., k]) & (P[..., k] < hi[k])
        pts = P[keep]
        with np.errstate(over="ignore"):
            xyz = pts.astype(np.float32) if dtype == "f32" else pts
        index = flat[keep]
        out.append((xyz, None if col is None else col[b].reshape(-1, 4)[index], index))
    return out if batched else out[0]


def write_ply(path, xyz, color=None):
    """A binary little-endian PLY of N points: `float x y z` (xyz [N,3], cast to float32), with color (uint8 [N,4], BGRA as the rig's
    colours) also `uchar red green blue`."""
    xyz = np.asarray(xyz)
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise ValueError("xyz must be [N,3], got shape %s" % (xyz.shape,))
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(xyz), "property float x", "property float y", "property float z"]
    if color is not None:
        color = np.asarray(color)
        if color.dtype != np.uint8 or color.shape != (len(xyz), 4):
            raise ValueError("color must be uint8 [N,4] (BGRA), got %s %s" % (color.dtype, color.shape))
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.empty(len(xyz), dtype=np.dtype(fields))
    with np.errstate(over="ignore"):
        rec["x"], rec["y"], rec["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if color is not None:
        rec["red"], rec["green"], rec["blue"] = color[:, 2], color[:, 1], color[:, 0]
    with open(path, "wb") as f:
        f.write(("\n".join(header + ["end_header"]) + "\n").encode("ascii"))
        f.write(rec.tobytes())


VOXEL_CELLS_MAX = 2 ** 20      # cells per axis: a cell index fits an int32, the packed key 60 bits
VOXEL_CAPACITY_MAX = 2 ** 26   # rows per pair the C entry takes
VOXEL_MIN_CAPACITY = 512       # the table is never smaller than for this capacity


def voxel_grid(size, lo, hi, step=1, disparity="d1", dtype="f32", capacity=None):
    """(lo float64 [3], hi float64 [3], size float, cells int64 [3]) of a voxel-cloud request after the checks
    sv_voxel_disparity_device makes (ValueError for a bad argument): compact_cloud's, and lo / hi / size finite, lo < hi, size > 0,
    cells[k] = max(1, ceil((hi[k] - lo[k]) / size)) <= 2^20, capacity None or an integer in 1 .. 2^26."""
    if lo is None or hi is None:
        raise ValueError("a voxel cloud needs a finite crop: lo and hi")
    lo, hi = cloud_crop(lo, hi, step, disparity, dtype)
    try:
        size = float(size)
    except (TypeError, ValueError):
        raise ValueError("size must be a number, got %r" % (size,))
    if not (np.isfinite(size) and size > 0):
        raise ValueError("size must be finite and > 0, got %r" % (size,))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise ValueError("the crop of a voxel cloud must be finite, got %r / %r" % (lo.tolist(), hi.tolist()))
    with np.errstate(over="ignore"):
        cells = np.ceil((hi - lo) / np.float64(size))
    if not (cells <= VOXEL_CELLS_MAX).all():
        raise ValueError("more than 2^20 cells on an axis: %r" % (cells.tolist(),))
    if capacity is not None and (isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= capacity <= VOXEL_CAPACITY_MAX):
        raise ValueError("capacity must be an integer in 1 .. 2^26, got %r" % (capacity,))
    return lo, hi, size, np.maximum(cells, 1).astype(np.int64)


def voxel_table_slots(capacity):
    """Entries of the table sv_voxel_disparity_device uses per pair (sv_voxel_table_slots): the power of two >= 2 * max(capacity, 512)."""
    if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= capacity <= VOXEL_CAPACITY_MAX:
        raise ValueError("capacity must be an integer in 1 .. 2^26, got %r" % (capacity,))
    slots = 1024
    while slots < 2 * max(int(capacity), VOXEL_MIN_CAPACITY):
        slots *= 2
    return slots


def voxel_cloud(disp, Q, size, lo, hi, XR=None, XT=None, step=1, disparity="d1", dtype="f32", colors=None, capacity=None):
    """Voxel-grid downsampled cloud(s), the definition of include/stereo_vision_hip.h (I) in numpy.

    The kept pixels are compact_cloud's (same disp, Q, XR / XT, lo / hi, step, disparity); lo / hi must be finite.  A kept point P lies
    in the cell c = min(int(t), cells - 1) per axis, t = (P - lo) / size, at the offset u = min(int((t - c) * 65536), 65535) inside it.
    A voxel is the kept points of one cell: n of them, the smallest flat pixel index `first`, the integer sums S = sum u and C = sum of
    the colour channels.  The voxels are listed in ascending `first`.
    Returns (xyz [V,3] float32 or float64 - lo + (c + (S + 0.5 n) / (65536 n)) * size in double, as written; color uint8 [V,4] =
    (2 C + n) // (2 n) (None without colors [H,W,4]); cell int32 [V,3]; n int32 [V]; first int32 [V]; count) with count = V, or, for
    a capacity with V > capacity, count = -1 and no rows - what the C entry reports.  For batched input a list of such tuples, one per
    frame.  write_ply takes xyz and color as they are."""
    lo, hi, size, cells = voxel_grid(size, lo, hi, step, disparity, dtype, capacity)
    d = np.asarray(disp, dtype=np.float32)
    batched = d.ndim == 3
    frames = compact_cloud(d, Q, XR, XT, lo, hi, step, disparity, "f64", colors)
    out = []
    for P, col, index in (frames if batched else [frames]):
        t = (P - lo) / np.float64(size)
        c = np.minimum(t.astype(np.int64), cells - 1)
        u = np.minimum(((t - c.astype(np.float64)) * 65536.0).astype(np.int64), 65535)
        key = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
        _, where, inverse, n = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
        order = np.argsort(where)  # index ascends with the row, so the first row of a voxel is its smallest pixel index
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        row = rank[inverse.reshape(-1)]  # of each point
        V = len(order)
        if capacity is not None and V > capacity:
            out.append((np.zeros((0, 3), np.float32 if dtype == "f32" else np.float64), None if col is None else np.zeros((0, 4), np.uint8),
                        np.zeros((0, 3), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), -1))
            continue
        n, where = n[order].astype(np.int64), where[order]
        S = np.zeros((V, 3), np.int64)
        np.add.at(S, row, u)
        nf = n.astype(np.float64)[:, None]
        xyz = lo + (c[where].astype(np.float64) + (S.astype(np.float64) + 0.5 * nf) / (65536.0 * nf)) * np.float64(size)
        color = None
        if col is not None:
            C = np.zeros((V, 4), np.int64)
            np.add.at(C, row, col.astype(np.int64))
            color = ((2 * C + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
        out.append((xyz.astype(np.float32) if dtype == "f32" else xyz, color, c[where].astype(np.int32), n.astype(np.int32), index[where].astype(np.int32), V))
    return out if batched else out[0]


VOXEL_MAP_SEQ_MAX = 2 ** 31 - 2  # the largest sequence number of a frame


def voxel_map_slots(capacity):
    """Entries of the table of a voxel map of `capacity` voxels (sv_voxel_map_slots): voxel_table_slots' rule."""
    return voxel_table_slots(capacity)


def voxel_map_params(lo, hi, size, capacity):
    """The words of a world-fixed voxel map (sv_voxel_map_spec) as a dict - lo, hi (tuples of 3 floats), size, capacity, and cells (3 ints)
    = max(1, ceil((hi - lo) / size)) - after voxel_grid's checks (ValueError): lo / hi / size finite, lo < hi, size > 0, at most 2^20
    cells per axis, capacity an integer in 1 .. 2^26."""
    if capacity is None:
        raise ValueError("a voxel map needs a capacity in 1 .. 2^26")
    lo, hi, size, cells = voxel_grid(size, lo, hi, capacity=capacity)
    return {"lo": tuple(lo.tolist()), "hi": tuple(hi.tolist()), "size": size, "capacity": int(capacity), "cells": tuple(int(c) for c in cells)}


def voxel_map_pose(x, y, yaw, z=0.0):
    """float64 [..., 12] = R row-major, then t: the pose of a frame whose vehicle axes stand at (x, y, z) in the world, turned by yaw about
    the z axis - Pw = R Pf + t with R = [[c, -s, 0], [s, c, 0], [0, 0, 1]], c and s exactly occupancy_pose's, so the same odometry drives
    both maps.  voxel_map_insert takes any rigid R | t in this layout as it is."""
    p = occupancy_pose(x, y, yaw)
    tx, ty, c, s = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    z = np.broadcast_to(np.asarray(z, np.float64), tx.shape)
    zero, one = np.zeros_like(tx), np.ones_like(tx)
    return np.stack([c, -s, zero, s, c, zero, zero, zero, one, tx, ty, z], -1)


def voxel_map_pose_words(poses):
    """float64 [B,12] from [B,12] poses (as they are) or the occupancy map's [B,4] = (tx, ty, c, s) (expanded as voxel_map_pose does,
    z = 0)."""
    p = np.asarray(poses, np.float64)
    if p.ndim == 1:
        p = p[None]
    if p.ndim != 2 or p.shape[1] not in (4, 12):
        raise ValueError("poses must be [B,12] or [B,4], got shape %s" % (p.shape,))
    if p.shape[1] == 12:
        return np.ascontiguousarray(p)
    zero, one = np.zeros(len(p)), np.ones(len(p))
    return np.stack([p[:, 2], -p[:, 3], zero, p[:, 3], p[:, 2], zero, zero, zero, one, p[:, 0], p[:, 1], zero], -1)


def voxel_map_slot_of(key, slots):
    """The slot at which the table's probing for `key` starts (sv_voxel_map_slot_of): (key * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2
    slots), slots a power of two in 2 .. 2^32.  int64, of key's shape."""
    if isinstance(slots, bool) or int(slots) != slots or not 2 <= slots <= 2 ** 32 or int(slots) & (int(slots) - 1):
        raise ValueError("slots must be a power of two in 2 .. 2^32, got %r" % (slots,))
    k = np.asarray(key, np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = (k * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(64 - (int(slots).bit_length() - 1))
    return h.astype(np.int64)


def voxel_map_state(params):
    """An empty map: params (voxel_map_params' dict, checked again), no voxel, dropped 0, not overflowed."""
    w = voxel_map_params(params["lo"], params["hi"], params["size"], params["capacity"])
    return {"params": w, "key": np.zeros(0, np.int64), "n": np.zeros(0, np.int64), "S": np.zeros((0, 3), np.int64), "C": np.zeros((0, 4), np.int64),
            "m": np.zeros(0, np.int64), "first_seq": np.zeros(0, np.int64), "last_seq": np.zeros(0, np.int64), "dropped": 0, "overflowed": False}


def _voxel_map_world(xyz, poses):
    """float64 [B,cap,3]: the rows xyz [B,cap,3], widened exactly to double, under the poses [B,12] - Pw[k] = ((R[k,0] x + R[k,1] y) +
    R[k,2] z) + t[k], in double and in that order: the insert's transform, which place_descriptor shares.  The caller holds np.errstate."""
    R = poses[:, None, :]
    P = xyz.astype(np.float64)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    return np.stack([((R[..., 3 * k] * x + R[..., 3 * k + 1] * y) + R[..., 3 * k + 2] * z) + R[..., 9 + k] for k in range(3)], -1)


def voxel_map_insert(map_state, xyz, color, n, counts, poses, seq0=0):
    """Adds B frames of rows to a world-fixed voxel map, the definition of include/stereo_vision_hip.h (Q) in numpy; map_state
    (voxel_map_state's dict) is changed in place and returned.

    xyz float32 or float64 [B,cap,3], color uint8 [B,cap,4] or None, n int32 [B,cap] or None (every weight 1), counts int32 [B] - what
    voxel_cloud_from_disparity and compact_cloud_from_disparity return -, poses float64 [B,12] (voxel_map_pose's layout).  Frame b
    contributes its first min(counts[b], cap) rows (none for counts[b] < 0).  A row (x, y, z), widened exactly to double, lies in the
    world at Pw[k] = ((R[k,0] x + R[k,1] y) + R[k,2] z) + t[k], in double and in that order.  It is dropped - and counted in
    map_state["dropped"] - when its weight w <= 0 or lo < Pw < hi does not hold strictly on every axis (NaN and inf never pass).  A kept
    row lies per axis in the cell c = min(int(t), cells - 1), t = (Pw - lo) / size, at the offset u = min(int((t - c) * 65536), 65535),
    and adds to the voxel of its cell n += w, S += w u, C += w colour, m += 1, first_seq = min(., seq0 + b), last_seq = max(., seq0 + b):
    all integers, 64-bit sums.  Contract: the total weight of a voxel stays below 2^47, 0 <= seq0 and seq0 + B - 1 <= 2^31 - 2.  A map
    that holds more than params["capacity"] voxels after the call is overflowed for good."""
    w = map_state["params"]
    lo, hi, size, cells = np.array(w["lo"]), np.array(w["hi"]), np.float64(w["size"]), np.array(w["cells"], np.int64)
    xyz = np.asarray(xyz)
    if xyz.dtype not in (np.float32, np.float64) or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be float32 or float64 [B,cap,3], got %s %s" % (xyz.dtype, xyz.shape))
    B, cap = xyz.shape[:2]
    counts = np.asarray(counts)
    poses = np.asarray(poses, np.float64)
    if counts.shape != (B,) or poses.shape != (B, 12):
        raise ValueError("counts must be [B] and poses [B,12] for B = %d, got %s and %s" % (B, counts.shape, poses.shape))
    if color is not None and (np.asarray(color).dtype != np.uint8 or np.asarray(color).shape != (B, cap, 4)):
        raise ValueError("color must be uint8 [B,cap,4] or None")
    if n is not None and np.asarray(n).shape != (B, cap):
        raise ValueError("n must be [B,cap] or None")
    if isinstance(seq0, bool) or int(seq0) != seq0 or seq0 < 0 or seq0 + B - 1 > VOXEL_MAP_SEQ_MAX:
        raise ValueError("the sequence numbers seq0 .. seq0 + B - 1 must stay in 0 .. 2^31 - 2, got seq0 = %r" % (seq0,))
    rows = np.arange(cap)[None, :] < np.minimum(counts.astype(np.int64), cap)[:, None]  # [B,cap]: the rows a frame contributes
    with np.errstate(invalid="ignore", over="ignore"):  # rows beyond counts may hold anything
        Pw = _voxel_map_world(xyz, poses)
        inside = ((lo < Pw) & (Pw < hi)).all(-1)
    wt = np.ones((B, cap), np.int64) if n is None else np.asarray(n).astype(np.int64)
    keep = rows & inside & (wt > 0)
    map_state["dropped"] += int((rows & ~keep).sum())
    b_of = np.broadcast_to(np.arange(B, dtype=np.int64)[:, None], (B, cap))[keep]
    t = (Pw[keep] - lo) / size
    c = np.minimum(t.astype(np.int64), cells - 1)
    u = np.minimum(((t - c.astype(np.float64)) * 65536.0).astype(np.int64), 65535)
    key = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
    wk = wt[keep]
    col = np.zeros((len(key), 4), np.int64) if color is None else np.asarray(color)[keep].astype(np.int64)
    seq = int(seq0) + b_of
    allkey = np.concatenate([map_state["key"], key])
    ukey, inv = np.unique(allkey, return_inverse=True)
    inv = inv.reshape(-1)
    V = len(ukey)
    acc = {"n": np.zeros(V, np.int64), "S": np.zeros((V, 3), np.int64), "C": np.zeros((V, 4), np.int64), "m": np.zeros(V, np.int64),
           "first_seq": np.full(V, np.iinfo(np.int64).max), "last_seq": np.full(V, -1, np.int64)}
    old, new = inv[:len(map_state["key"])], inv[len(map_state["key"]):]
    for f in ("n", "S", "C", "m", "first_seq", "last_seq"):
        acc[f][old] = map_state[f]
    np.add.at(acc["n"], new, wk)
    np.add.at(acc["S"], new, wk[:, None] * u)
    np.add.at(acc["C"], new, wk[:, None] * col)
    np.add.at(acc["m"], new, 1)
    np.minimum.at(acc["first_seq"], new, seq)
    np.maximum.at(acc["last_seq"], new, seq)
    map_state.update(acc, key=ukey)
    if V > w["capacity"]:
        map_state["overflowed"] = True
    return map_state


def voxel_map_rows(map_state, min_n=1, min_rows=1, since=0, dtype="f32"):
    """The voxels of a map with n >= min_n, m >= min_rows and last_seq >= since, in ascending key cx | cy << 20 | cz << 40, as a dict:
    xyz [V,3] float32 or float64 ("f64") = lo + (c + (S + 0.5 n) / (65536 n)) * size in double, as written; color uint8 [V,4] =
    (2 C + n) // (2 n); cell int32 [V,3]; n int64 [V]; m int64 [V]; first_seq, last_seq int32 [V]; key int64 [V]; count = V.  An
    overflowed map reports count -1 and no rows."""
    if dtype not in CLOUD_DTYPES:
        raise ValueError("dtype must be one of %s, got %r" % (sorted(CLOUD_DTYPES), dtype))
    w = map_state["params"]
    sel = (map_state["n"] >= min_n) & (map_state["m"] >= min_rows) & (map_state["last_seq"] >= since)
    if map_state["overflowed"]:
        sel = np.zeros(0, bool)
    key = map_state["key"][sel] if len(sel) else np.zeros(0, np.int64)
    pick = (lambda f: map_state[f][sel]) if len(sel) else (lambda f: map_state[f][:0])
    n, S, C = pick("n"), pick("S"), pick("C")
    c = np.stack([key & 0xFFFFF, (key >> 20) & 0xFFFFF, (key >> 40) & 0xFFFFF], -1)
    nf = n.astype(np.float64)[:, None]
    xyz = np.array(w["lo"]) + (c.astype(np.float64) + (S.astype(np.float64) + 0.5 * nf) / (65536.0 * nf)) * np.float64(w["size"])
    return {"xyz": xyz.astype(np.float32) if dtype == "f32" else xyz, "color": ((2 * C + n[:, None]) // (2 * n[:, None])).astype(np.uint8),
            "cell": c.astype(np.int32), "n": n, "m": pick("m"), "first_seq": pick("first_seq").astype(np.int32), "last_seq": pick("last_seq").astype(np.int32),
            "key": key, "count": -1 if map_state["overflowed"] else int(len(key))}


VOXEL_CARRY_SHIFT_MAX = 2 ** 20   # |shift| per axis of voxel_map_carry: an axis has at most that many cells
VOXEL_CARRY_STATS = ("carried", "filtered", "outside", "claimed")  # voxel_map_carry's counts, in the order of the C entry's stats
VOXEL_MERGE_TOLERANCE = 1.0 / 65536  # cells: how far the boxes of two maps that merge may miss a whole number of cells
_VOXEL_SHIFT_ULPS = 4              # how far voxel_map_shifted moves hi' to keep the count of cells


def _whole(v, what):
    """int(v) for an integer that is no bool; ValueError otherwise."""
    try:
        ok = not isinstance(v, (bool, np.bool_)) and int(v) == v
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("%s must be an integer, got %r" % (what, v))
    return int(v)


def _voxel_map_cells_of(lo, hi, size):
    """max(1, ceil((hi - lo) / size)) as voxel_grid computes it, for one axis."""
    return max(1, int(np.ceil((np.float64(hi) - np.float64(lo)) / np.float64(size))))


def voxel_map_shifted(params, shift_cells, capacity=None):
    """The params of the box of `params` moved by shift_cells = (kx, ky, kz) whole cells, with the capacity given or the same: per axis lo' =
    lo + k * size in double (the product rounded, then the sum), hi' = lo' + (hi - lo), and `cells` identical to the source's.  That last
    is not automatic - cells = max(1, ceil((hi' - lo') / size)) is recomputed from rounded doubles -, so hi' is moved by up to 4 ulps,
    towards the count wanted, until it is; ValueError where that does not get there, where a k is not an integer below 2^31 in magnitude,
    or where the moved box is not one voxel_map_params admits.

    voxel_map_carry into the moved box takes shift = -k.  The position voxel_map_rows reports for a carried voxel is then lo' + (c - k + f)
    * size in place of lo + (c + f) * size (f the voxel's mean offset as a fraction of a cell, the same double in both).  The two agree
    in exact arithmetic; as computed they differ by the roundings of k * size, of lo + k size, and of the sum, the product and the sum of
    either position: with u = 2^-53, per axis and for dtype "f64",
        |p' - p| <= 1.01 u (|k| size + |lo'| + 2 (c + 1) size + 2 (c - k + 1) size + |p| + |p'|)
    (voxel_map_shift_bound) - a few 1e-14 m for a box of a hundred metres a thousand cells from where it started."""
    w = voxel_map_params(params["lo"], params["hi"], params["size"], params["capacity"] if capacity is None else capacity)
    if not isinstance(shift_cells, (tuple, list, np.ndarray)):
        raise ValueError("shift_cells must be three integers, got %r" % (shift_cells,))
    k = [_whole(v, "a shift of voxel_map_shifted") for v in shift_cells]
    if len(k) != 3 or max(abs(v) for v in k) >= 2 ** 31:
        raise ValueError("shift_cells must be three integers below 2^31 in magnitude, got %r" % (shift_cells,))
    size = np.float64(w["size"])
    lo, hi = np.array(w["lo"], np.float64), np.array(w["hi"], np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        lo2 = lo + np.array(k, np.float64) * size
        hi2 = lo2 + (hi - lo)
    if not (np.isfinite(lo2).all() and np.isfinite(hi2).all()):
        raise ValueError("the box moved by %r cells is not finite" % (k,))
    for a in range(3):
        want = w["cells"][a]
        for _ in range(_VOXEL_SHIFT_ULPS):
            have = _voxel_map_cells_of(lo2[a], hi2[a], size)
            if have == want:
                break
            hi2[a] = np.nextafter(hi2[a], -np.inf if have > want else np.inf)
        if _voxel_map_cells_of(lo2[a], hi2[a], size) != want:
            raise ValueError("the box moved by %r cells cannot keep its %d cells on axis %d" % (k, want, a))
    moved = voxel_map_params(lo2, hi2, w["size"], w["capacity"])
    if moved["cells"] != w["cells"]:
        raise ValueError("the box moved by %r cells has %r cells, not %r" % (k, moved["cells"], w["cells"]))
    return moved


def voxel_map_shift_bound(params, moved, shift_cells, cell, p, p_moved):
    """The bound voxel_map_shifted's docstring derives, per axis: float64 [..., 3] for cells `cell` (int [..., 3], in the box of `params`)
    whose positions are p in that box and p_moved in `moved` = voxel_map_shifted(params, shift_cells)."""
    k = np.array(shift_cells, np.float64)
    c = np.asarray(cell, np.float64)
    size = np.float64(params["size"])
    return 1.01 * 2.0 ** -53 * (np.abs(k) * size + np.abs(np.array(moved["lo"])) + 2 * (c + 1) * size + 2 * (c - k + 1) * size
                                + np.abs(np.asarray(p, np.float64)) + np.abs(np.asarray(p_moved, np.float64)))


def voxel_map_recenter_shift(params, x, y, z=None):
    """(kx, ky, kz): the whole cells by which the box of `params` must move (voxel_map_shifted) so that the world point (x, y, z) lies in
    its middle cell (cells // 2 per axis) - occupancy_recenter_shift's rule on three axes.  The point's cell is floor((p - lo) / size),
    so k = floor((p - lo) / size) - cells // 2; z = None leaves the z axis alone (kz = 0).  ValueError for a point that is not finite or
    lies 2^31 cells or more from the box."""
    w = voxel_map_params(params["lo"], params["hi"], params["size"], params["capacity"])
    k = []
    for a, p in enumerate((x, y, z)):
        if p is None and a == 2:
            k.append(0)
            continue
        if p is None or not np.isfinite(p):
            raise ValueError("recenter needs a finite point, got (%r, %r, %r)" % (x, y, z))
        with np.errstate(over="ignore"):
            t = np.floor((np.float64(p) - np.float64(w["lo"][a])) / np.float64(w["size"]))
        if not abs(t) < 2.0 ** 31:
            raise ValueError("the point (%r, %r, %r) lies 2^31 cells or more from the box" % (x, y, z))
        k.append(int(t) - w["cells"][a] // 2)
    return tuple(k)


def voxel_map_carry(dst_state, src_state, shift=(0, 0, 0), min_n=1, min_rows=1, since=0):
    """Adds the voxels of one voxel map, filtered and shifted by whole cells, into another: the definition of include/stereo_vision_hip.h
    (S) in numpy.  dst_state (voxel_map_state's dict) is changed in place, src_state is only read; -> a dict of counts.

    The two maps must be distinct and of bit-equal `size`; shift is three integers in -2^20 .. 2^20 (ValueError otherwise).  A voxel of
    src qualifies iff n >= min_n, m >= min_rows and last_seq >= since - voxel_map_rows' filters -; one that does not counts into
    "filtered".  A qualifying voxel whose cell c + shift leaves 0 .. cells - 1 of dst on an axis counts into "outside".  Every other
    voxel is carried: the voxel of dst with the key of c + shift gets n += n, S += S, C += C, m += m, first_seq = min(., first_seq),
    last_seq = max(., last_seq) - S as it is: whole cells do not move a point inside its cell.  "carried" counts them, "claimed" those
    dst did not hold before.  dst["dropped"] += src["dropped"].  dst is overflowed afterwards iff it was before, or src is, or it now
    holds more than its capacity.  Where src or dst is overflowed as the call starts nothing is carried: "carried" is -1 - as
    voxel_map_rows' count - and the other counts 0.  Contract: the total weight of a voxel of dst stays below 2^47.

    An empty dst of the same box makes this a prune, a box moved by k cells (voxel_map_shifted; shift = -k) a scroll, a larger capacity
    a grow, a dst that holds voxels a merge."""
    if dst_state is src_state:
        raise ValueError("voxel_map_carry needs two distinct maps")
    ws, wd = src_state["params"], dst_state["params"]
    if np.float64(ws["size"]).tobytes() != np.float64(wd["size"]).tobytes():
        raise ValueError("the two maps differ in size: %r and %r" % (ws["size"], wd["size"]))
    if not isinstance(shift, (tuple, list, np.ndarray)):
        raise ValueError("shift must be three integers, got %r" % (shift,))
    shift = [_whole(v, "a shift of voxel_map_carry") for v in shift]
    if len(shift) != 3 or max(abs(v) for v in shift) > VOXEL_CARRY_SHIFT_MAX:
        raise ValueError("shift must be three integers in -2^20 .. 2^20, got %r" % (shift,))
    for v, what in ((min_n, "min_n"), (min_rows, "min_rows"), (since, "since")):
        if isinstance(v, bool) or int(v) != v:
            raise ValueError("%s must be an integer, got %r" % (what, v))
    stats = dict.fromkeys(VOXEL_CARRY_STATS, 0)
    dst_state["dropped"] += src_state["dropped"]
    if src_state["overflowed"] or dst_state["overflowed"]:
        dst_state["overflowed"] = True
        stats["carried"] = -1
        return stats
    q = (src_state["n"] >= min_n) & (src_state["m"] >= min_rows) & (src_state["last_seq"] >= since)
    key = src_state["key"]
    c = np.stack([key & 0xFFFFF, (key >> 20) & 0xFFFFF, (key >> 40) & 0xFFFFF], -1) + np.array(shift, np.int64)
    inside = ((c >= 0) & (c < np.array(wd["cells"], np.int64))).all(-1)
    take = q & inside
    stats["filtered"], stats["outside"], stats["carried"] = int((~q).sum()), int((q & ~inside).sum()), int(take.sum())
    c = c[take]
    moved = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)  # distinct: src's keys are, and the shift is the same for all
    had = len(dst_state["key"])
    ukey, inv = np.unique(np.concatenate([dst_state["key"], moved]), return_inverse=True)
    inv = inv.reshape(-1)
    V = len(ukey)
    acc = {"n": np.zeros(V, np.int64), "S": np.zeros((V, 3), np.int64), "C": np.zeros((V, 4), np.int64), "m": np.zeros(V, np.int64),
           "first_seq": np.full(V, np.iinfo(np.int64).max), "last_seq": np.full(V, -1, np.int64)}
    old, new = inv[:had], inv[had:]
    for f in ("n", "S", "C", "m", "first_seq", "last_seq"):
        acc[f][old] = dst_state[f]
    for f in ("n", "S", "C", "m"):
        acc[f][new] += src_state[f][take]
    acc["first_seq"][new] = np.minimum(acc["first_seq"][new], src_state["first_seq"][take])
    acc["last_seq"][new] = np.maximum(acc["last_seq"][new], src_state["last_seq"][take])
    dst_state.update(acc, key=ukey)
    stats["claimed"] = V - had
    if V > wd["capacity"]:
        dst_state["overflowed"] = True
    return stats


VOXEL_REPOSE_CORR_MAX = 2 ** 22  # corrections per call of voxel_map_repose


def _voxel_repose_setup(dst_state, src_state, corr, seq0, min_n, min_rows, since):
    """voxel_map_repose's checks (ValueError) -> (corr float64 [K,12], seq0, min_n, min_rows, since) as the definition takes them."""
    if dst_state is src_state:
        raise ValueError("voxel_map_repose needs two distinct maps")
    try:
        corr = np.ascontiguousarray(corr, np.float64)
    except (TypeError, ValueError):
        raise ValueError("corr must be float64 [K,12]")
    if corr.ndim != 2 or corr.shape[1] != 12 or not 1 <= corr.shape[0] <= VOXEL_REPOSE_CORR_MAX:
        raise ValueError("corr must be float64 [K,12] with K in 1 .. 2^22, got shape %s" % (corr.shape,))
    seq0 = _whole(seq0, "seq0")
    if not 0 <= seq0 <= VOXEL_MAP_SEQ_MAX:
        raise ValueError("seq0 must be an integer in 0 .. 2^31 - 2, got %r" % (seq0,))
    return corr, seq0, _whole(min_n, "min_n"), _whole(min_rows, "min_rows"), _whole(since, "since")


def voxel_map_repose(dst_state, src_state, corr, seq0=0, min_n=1, min_rows=1, since=0):
    """Adds the voxels of one voxel map, each moved by the rigid correction of the frame that saw it last, into another: the definition
    of include/stereo_vision_hip.h (AD) in numpy.  dst_state (voxel_map_state's dict) is changed in place, src_state is only read; -> a
    dict of counts in VOXEL_CARRY_STATS' order.

    The two maps must be distinct; box, size and capacity may all differ.  corr is float64 [K,12] in voxel_map_pose's layout, K in 1 ..
    2^22, any twelve words taken as they are (as the insert takes any pose); seq0 an integer in 0 .. 2^31 - 2 (ValueError otherwise).  A
    voxel of src qualifies iff n >= max(min_n, 1), m >= min_rows and last_seq >= since; one that does not counts into "filtered" - a
    tombstone (n = 0, what carve and despeckle leave) never qualifies, whatever min_n is: the next step divides by n.  A qualifying
    voxel stands at p, the read-out's centre (voxel_map_rows' xyz for "f64", as written there), and is moved by corr[k], k = min(max(
    last_seq - seq0, 0), K - 1): last_seq is the one rule, so a voxel that two passes of a drive share is moved with the later pass.  Pw
    = _voxel_map_world(p, corr[k]), the insert's transform in its order, no FMA.  Where lo < Pw < hi of dst fails strictly on an axis
    the voxel counts into "outside" - NaN and inf never pass, so neither does a correction that is not finite.  Every other voxel is
    carried: with the insert's cell c = min(int(t), cells - 1), t = (Pw - lo) / size, and offset u = min(int((t - c) * 65536), 65535) the
    voxel of dst with c's key gets n += n, S += n u, C += C, m += m, first_seq = min(., first_seq), last_seq = max(., last_seq): an
    insert of one row of weight n at the voxel's mean, with the carry's bookkeeping.  "carried" counts them, "claimed" the voxels dst
    did not hold before.  The head is the carry's: dst["dropped"] += src["dropped"]; where src or dst is overflowed as the call starts
    nothing is carried, "carried" is -1 and the other counts 0; dst is overflowed afterwards iff it was, or src is, or it now holds
    more than its capacity.  Contract: the total weight of a voxel of dst stays below 2^47.

    There is no shortcut for the identity: a voxel's points collapse to their mean, and S becomes n times a whole offset - floor(S / n + 1 / 2), the centre's -, so a re-pose
    costs up to 1 / 65536 of a cell of position, once per call, whatever the corrections are."""
    corr, seq0, min_n, min_rows, since = _voxel_repose_setup(dst_state, src_state, corr, seq0, min_n, min_rows, since)
    ws, wd = src_state["params"], dst_state["params"]
    stats = dict.fromkeys(VOXEL_CARRY_STATS, 0)
    dst_state["dropped"] += src_state["dropped"]
    if src_state["overflowed"] or dst_state["overflowed"]:
        dst_state["overflowed"] = True
        stats["carried"] = -1
        return stats
    q = (src_state["n"] >= max(min_n, 1)) & (src_state["m"] >= min_rows) & (src_state["last_seq"] >= since)
    key, n = src_state["key"][q], src_state["n"][q]
    c = np.stack([key & 0xFFFFF, (key >> 20) & 0xFFFFF, (key >> 40) & 0xFFFFF], -1)
    nf = n.astype(np.float64)[:, None]
    p = np.array(ws["lo"]) + (c.astype(np.float64) + (src_state["S"][q].astype(np.float64) + 0.5 * nf) / (65536.0 * nf)) * np.float64(ws["size"])
    k = np.clip(src_state["last_seq"][q].astype(np.int64) - seq0, 0, len(corr) - 1)
    lo, hi, size, cells = np.array(wd["lo"]), np.array(wd["hi"]), np.float64(wd["size"]), np.array(wd["cells"], np.int64)
    with np.errstate(invalid="ignore", over="ignore"):  # a correction may hold anything
        Pw = _voxel_map_world(p[:, None, :], corr[k])[:, 0, :]
        inside = ((lo < Pw) & (Pw < hi)).all(-1)
    stats["filtered"], stats["outside"], stats["carried"] = int((~q).sum()), int((~inside).sum()), int(inside.sum())
    t = (Pw[inside] - lo) / size
    c = np.minimum(t.astype(np.int64), cells - 1)
    u = np.minimum(((t - c.astype(np.float64)) * 65536.0).astype(np.int64), 65535)
    moved = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
    take = np.flatnonzero(q)[inside]
    had = len(dst_state["key"])
    ukey, inv = np.unique(np.concatenate([dst_state["key"], moved]), return_inverse=True)
    inv = inv.reshape(-1)
    V = len(ukey)
    acc = {"n": np.zeros(V, np.int64), "S": np.zeros((V, 3), np.int64), "C": np.zeros((V, 4), np.int64), "m": np.zeros(V, np.int64),
           "first_seq": np.full(V, np.iinfo(np.int64).max), "last_seq": np.full(V, -1, np.int64)}
    old, new = inv[:had], inv[had:]
    for f in ("n", "S", "C", "m", "first_seq", "last_seq"):
        acc[f][old] = dst_state[f]
    nk = src_state["n"][take]
    np.add.at(acc["n"], new, nk)
    np.add.at(acc["S"], new, nk[:, None] * u)
    np.add.at(acc["C"], new, src_state["C"][take])
    np.add.at(acc["m"], new, src_state["m"][take])
    np.minimum.at(acc["first_seq"], new, src_state["first_seq"][take])
    np.maximum.at(acc["last_seq"], new, src_state["last_seq"][take])
    dst_state.update(acc, key=ukey)
    stats["claimed"] = V - had
    if V > wd["capacity"]:
        dst_state["overflowed"] = True
    return stats


def voxel_map_repose_brute(dst_state, src_state, corr, seq0=0, min_n=1, min_rows=1, since=0):
    """voxel_map_repose voxel by voxel: a Python loop over the entries of src with a dict for dst, Python floats and ints only."""
    corr, seq0, min_n, min_rows, since = _voxel_repose_setup(dst_state, src_state, corr, seq0, min_n, min_rows, since)
    ws, wd = src_state["params"], dst_state["params"]
    stats = dict.fromkeys(VOXEL_CARRY_STATS, 0)
    dst_state["dropped"] += src_state["dropped"]
    if src_state["overflowed"] or dst_state["overflowed"]:
        dst_state["overflowed"] = True
        stats["carried"] = -1
        return stats
    fields = ("n", "S", "C", "m", "first_seq", "last_seq")
    vox = {int(key): [dst_state[f][i].tolist() for f in fields] for i, key in enumerate(dst_state["key"])}
    had = len(vox)
    for i, key in enumerate(src_state["key"].tolist()):
        n, S, C, m, first, last = (src_state[f][i].tolist() for f in fields)
        if not (n >= max(min_n, 1) and m >= min_rows and last >= since):
            stats["filtered"] += 1
            continue
        w = [float(v) for v in corr[min(max(last - seq0, 0), len(corr) - 1)]]
        p = [ws["lo"][a] + (float((key >> (20 * a)) & 0xFFFFF) + (float(S[a]) + 0.5 * float(n)) / (65536.0 * float(n))) * float(ws["size"]) for a in range(3)]
        moved, u = 0, []
        for a in range(3):
            with np.errstate(invalid="ignore", over="ignore"):  # numpy scalars: inf and NaN by IEEE, where Python floats would raise
                P = float(((np.float64(w[3 * a]) * p[0] + np.float64(w[3 * a + 1]) * p[1]) + np.float64(w[3 * a + 2]) * p[2]) + np.float64(w[9 + a]))
            if not (wd["lo"][a] < P < wd["hi"][a]):  # false for NaN, and for inf: lo and hi are finite
                moved = None
                break
            t = (P - wd["lo"][a]) / float(wd["size"])
            c = min(int(t), wd["cells"][a] - 1)
            u.append(min(int((t - float(c)) * 65536.0), 65535))
            moved |= c << (20 * a)
        if moved is None:
            stats["outside"] += 1
            continue
        stats["carried"] += 1
        v = vox.setdefault(moved, [0, [0, 0, 0], [0, 0, 0, 0], 0, None, None])
        v[0] += n
        v[1] = [v[1][a] + n * u[a] for a in range(3)]
        v[2] = [v[2][j] + C[j] for j in range(4)]
        v[3] += m
        v[4], v[5] = first if v[4] is None else min(v[4], first), last if v[5] is None else max(v[5], last)
    keys = sorted(vox)
    V = len(keys)
    dst_state.update(key=np.array(keys, np.int64).reshape(V), n=np.array([vox[k][0] for k in keys], np.int64).reshape(V),
                     S=np.array([vox[k][1] for k in keys], np.int64).reshape(V, 3), C=np.array([vox[k][2] for k in keys], np.int64).reshape(V, 4),
                     m=np.array([vox[k][3] for k in keys], np.int64).reshape(V), first_seq=np.array([vox[k][4] for k in keys], np.int64).reshape(V),
                     last_seq=np.array([vox[k][5] for k in keys], np.int64).reshape(V))
    stats["claimed"] = V - had
    if V > wd["capacity"]:
        dst_state["overflowed"] = True
    return stats


def _pose_mul(a, b):
    """a o b of two [12] motions (R row-major, then t): (Ra Rb | Ra tb + ta), in double."""
    Ra, Rb = a[:9].reshape(3, 3), b[:9].reshape(3, 3)
    return np.concatenate([(Ra @ Rb).reshape(9), Ra @ b[9:] + a[9:]])


def _pose_inv(a):
    """The rigid inverse (R^T | -R^T t) of a [12] motion."""
    Rt = a[:9].reshape(3, 3).T
    return np.concatenate([Rt.reshape(9), -(Rt @ a[9:])])


def _pose_V(om, angle):
    """The matrix V of se(3)'s exponential: exp((om, v)) = (exp(om) | V v)."""
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    if angle > 1e-2:
        return np.eye(3) + ((1.0 - np.cos(angle)) / (angle * angle)) * K + ((angle - np.sin(angle)) / (angle ** 3)) * (K @ K)
    a2 = angle * angle  # the series: the closed forms cancel below; the terms left out are below 3e-17
    return np.eye(3) + (0.5 - a2 / 24.0 + a2 * a2 / 720.0) * K + (1.0 / 6.0 - a2 / 120.0 + a2 * a2 / 5040.0) * (K @ K)


def pose_exp(xi):
    """exp of xi = (om [3] radians, v [3]) in se(3) as a [12] motion: the rotation is _flow_exp's, the translation V(om) v."""
    xi = np.asarray(xi, np.float64).reshape(6)
    R, angle = _flow_exp(xi[:3])
    return np.concatenate([R.reshape(9), _pose_V(xi[:3], angle) @ xi[3:]])


def pose_log(pose):
    """log of a rigid [12] motion in se(3): (om, v) float64 [6] with pose_exp(pose_log(P)) = P.  ValueError for a rotation within 1e-6
    of pi, where the axis is not determined by R - R^T."""
    P = np.asarray(pose, np.float64).reshape(12)
    R = P[:9].reshape(3, 3)
    a = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])  # sin(angle) * axis
    s = float(np.sqrt((a * a).sum()))
    angle = float(np.arctan2(s, 0.5 * (np.trace(R) - 1.0)))
    if not np.isfinite(angle) or angle > np.pi - 1e-6:
        raise ValueError("the rotation is within 1e-6 of pi (or not finite): its logarithm is not determined")
    om = a * (angle / s) if s > 1e-12 else a
    return np.concatenate([om, np.linalg.solve(_pose_V(om, angle), P[9:])])


def _poses_12(poses, what):
    p = np.ascontiguousarray(poses, np.float64)
    if p.ndim != 2 or p.shape[1] != 12:
        raise ValueError("%s must be float64 [N,12], got shape %s" % (what, p.shape))
    return p


def pose_corrections(old, new):
    """float64 [N,12]: new[k] o old[k]^-1 with the rigid inverse (R^T | -R^T t) - what moves a world point placed under old[k] to where
    new[k] places it: the corrections voxel_map_repose and PlaceIndex.repose take, from pose_graph_optimize or any caller's pose graph.  old, new float64
    [N,12] rigid poses in voxel_map_pose's layout."""
    old, new = _poses_12(old, "old"), _poses_12(new, "new")
    if old.shape != new.shape:
        raise ValueError("old and new must hold one pose per frame each, got %s and %s" % (old.shape, new.shape))
    return np.ascontiguousarray(np.array([_pose_mul(new[k], _pose_inv(old[k])) for k in range(len(old))]).reshape(len(old), 12))


def loop_spread(poses, i, j, target, weights=None):
    """Spreads the error of one confirmed loop along the chain of poses: float64 [N,12] from poses [N,12], the frames i < j the loop
    ties and `target` [12], the pose frame j should have (the loop's: PlaceIndex.guess refined by VoxelMap.localize and .align).  E =
    poses[j]^-1 o target, xi = log E in se(3) (pose_log).  P'_k = P_k for k < i, bit for bit; P'_k = P_k o exp(f_k xi) for i <= k <= j, so
    P'_j = target; P'_k = target o P_j^-1 o P_k for k > j: the frames behind the loop keep their motions relative to frame j.  f_k = (k - i)
    / (j - i), or with weights - [j - i], the weight of the step from frame i + s to i + s + 1, or [N - 1], of every step of the chain; say
    the distance travelled - the cumulative weight from i to k over its total.  Not a solver: one loop, no covariance.  ValueError for i
    >= j or outside the chain, a rotation of E within 1e-6 of pi, and weights that are negative, not finite or sum to zero."""
    P = _poses_12(poses, "poses")
    N = len(P)
    i, j = _whole(i, "i"), _whole(j, "j")
    if not 0 <= i < j < N:
        raise ValueError("loop_spread needs 0 <= i < j < %d, got i = %d, j = %d" % (N, i, j))
    target = np.asarray(target, np.float64)
    if target.shape != (12,):
        raise ValueError("target must be float64 [12], got shape %s" % (target.shape,))
    if weights is None:
        f = np.arange(j - i + 1, dtype=np.float64) / float(j - i)
    else:
        w = np.asarray(weights, np.float64)
        if w.shape == (N - 1,) and N - 1 != j - i:
            w = w[i:j]
        if w.shape != (j - i,):
            raise ValueError("weights must be [%d] or [%d], got shape %s" % (j - i, N - 1, w.shape))
        if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
            raise ValueError("weights must be finite, not negative, and sum to more than zero")
        f = np.concatenate([[0.0], np.cumsum(w)]) / w.sum()
        f[-1] = 1.0
    xi = pose_log(_pose_mul(_pose_inv(P[j]), target))
    out = P.copy()
    for k in range(i, j + 1):
        out[k] = _pose_mul(P[k], pose_exp(f[k - i] * xi))
    tail = _pose_mul(target, _pose_inv(P[j]))
    for k in range(j + 1, N):
        out[k] = _pose_mul(tail, P[k])
    return out


def pose_repose(poses, seq, corr, seq0=0):
    """float64 [N,12]: corr[k] o poses[r] with k = min(max(seq[r] - seq0, 0), K - 1) - voxel_map_repose's index rule on the sequence
    numbers seq [N] of stored poses: what PlaceIndex.repose makes of its key poses."""
    P = _poses_12(poses, "poses")
    corr = _poses_12(corr, "corr")
    seq = np.asarray(seq, np.int64)
    seq0 = _whole(seq0, "seq0")
    if seq.shape != (len(P),) or not 1 <= len(corr) <= VOXEL_REPOSE_CORR_MAX or not 0 <= seq0 <= VOXEL_MAP_SEQ_MAX:
        raise ValueError("seq must be [%d], corr [K,12] with K in 1 .. 2^22 and seq0 in 0 .. 2^31 - 2" % len(P))
    k = np.clip(seq - seq0, 0, len(corr) - 1)
    return np.ascontiguousarray(np.array([_pose_mul(corr[k[r]], P[r]) for r in range(len(P))]).reshape(len(P), 12))


# ---- (AE) the pose graph of confirmed loops: batch least squares by Gauss-Newton rounds, each solved by preconditioned conjugate
# gradients.  Every double below is formed one operation at a time, in one stated order, with no fused multiply-add and no library sum:
# the numpy forms, the *_brute loops and the kernels of pose_graph_kernels.hip give the same bits.  Trigonometry (pose_exp) stays in
# pose_graph_optimize, which is host code shared by the CPU and the GPU path.

POSE_GRAPH_POSES_MAX = 1 << 20
POSE_GRAPH_EDGES_MAX = 1 << 22
POSE_GRAPH_CHUNK = 256   # poses per chunk of a dot product: a workgroup of the pose kernels
POSE_GRAPH_ROUND = 16    # PCG iterations the engine enqueues between two looks at the state words
POSE_GRAPH_ODOMETRY, POSE_GRAPH_LOOP = 0, 1
_PG_TRI = tuple((p, q) for p in range(6) for q in range(p + 1))          # the 21 words of a symmetric 6 x 6 block: row p, column q <= p
_PG_AT = {pq: n for n, pq in enumerate(_PG_TRI)}
_PG_DIAG = tuple(_PG_AT[(p, p)] for p in range(6))


def pose_graph_sum(v):
    """The sum every dot product of the pose graph ends in: the values in chunks of 256, zero padded, each chunk reduced by a halving
    tree - v[k] + v[k + h] for k < h, h = 128 .. 1 -, and the chunks' partials by the same rule until one value is left.  No value
    gives 0.0.  -> float."""
    v = np.ascontiguousarray(v, np.float64).reshape(-1)
    if v.size == 0:
        return 0.0
    while True:
        c = -(-v.size // POSE_GRAPH_CHUNK)
        a = np.zeros(c * POSE_GRAPH_CHUNK)
        a[:v.size] = v
        a = a.reshape(c, POSE_GRAPH_CHUNK)
        h = POSE_GRAPH_CHUNK // 2
        while h >= 1:
            a = a[:, :h] + a[:, h:2 * h]
            h //= 2
        v = a[:, 0]
        if c == 1:
            return float(v[0])


def pose_graph_sum_brute(v):
    v = [float(t) for t in np.asarray(v, np.float64).reshape(-1)]
    if not v:
        return 0.0
    while True:
        partials = []
        for c0 in range(0, len(v), POSE_GRAPH_CHUNK):
            a = v[c0:c0 + POSE_GRAPH_CHUNK]
            a += [0.0] * (POSE_GRAPH_CHUNK - len(a))
            h = POSE_GRAPH_CHUNK // 2
            while h >= 1:
                for k in range(h):
                    a[k] = a[k] + a[k + h]
                h //= 2
            partials.append(a[0])
        v = partials
        if len(v) == 1:
            return v[0]


def pose_graph_words(n_poses, i, j):
    """The incidence lists of a graph, CSR: -> row_start int32 [N + 1], inc int32 [2 E].  Pose k's entries are inc[row_start[k] :
    row_start[k + 1]], ascending; an entry is 2 e for edge e where k is its j, 2 e + 1 where k is its i.  A stable sort on the host."""
    i, j = np.asarray(i, np.int64).reshape(-1), np.asarray(j, np.int64).reshape(-1)
    pose = np.stack([j, i], 1).reshape(-1)
    order = np.argsort(pose, kind="stable")
    row_start = np.concatenate([[0], np.cumsum(np.bincount(pose, minlength=n_poses))])
    return row_start.astype(np.int32), order.astype(np.int32)


def _pg_mv(R, x):
    return np.stack([(R[..., 3 * a] * x[..., 0] + R[..., 3 * a + 1] * x[..., 1]) + R[..., 3 * a + 2] * x[..., 2] for a in range(3)], -1)


def _pg_mtv(R, x):
    return np.stack([(R[..., a] * x[..., 0] + R[..., 3 + a] * x[..., 1]) + R[..., 6 + a] * x[..., 2] for a in range(3)], -1)


def _pg_cross(t, u):
    return np.stack([t[..., 1] * u[..., 2] - t[..., 2] * u[..., 1], t[..., 2] * u[..., 0] - t[..., 0] * u[..., 2],
                     t[..., 0] * u[..., 1] - t[..., 1] * u[..., 0]], -1)


def _pg_ad(M, x):
    """Ad_M x of x = (om, v): (R om, t x (R om) + R v)."""
    u = _pg_mv(M[..., :9], x[..., :3])
    return np.concatenate([u, _pg_cross(M[..., 9:], u) + _pg_mv(M[..., :9], x[..., 3:])], -1)


def _pg_adt(M, g):
    """Ad_M^T g of g = (g_rot, g_trans): (R^T (g_rot - t x g_trans), R^T g_trans)."""
    return np.concatenate([_pg_mtv(M[..., :9], g[..., :3] - _pg_cross(M[..., 9:], g[..., 3:])), _pg_mtv(M[..., :9], g[..., 3:])], -1)


def _pg_dot6(a, b):
    s = a[..., 0] * b[..., 0]
    for c in range(1, 6):
        s = s + a[..., c] * b[..., c]
    return s


def _pg_ranks(row_start, inc):
    """The incidence lists by rank: [(poses with more than d entries, the edge of their d-th entry, whether they are its i)] for d = 0,
    1, ...: a pose occurs once per rank, so a rank is one vectorised step of every pose's left-to-right sum."""
    row_start, inc = np.asarray(row_start, np.int64), np.asarray(inc, np.int64)
    deg = np.diff(row_start)
    out = []
    for d in range(int(deg.max()) if deg.size else 0):
        k = np.nonzero(deg > d)[0]
        c = inc[row_start[k] + d]
        out.append((k, c >> 1, (c & 1).astype(bool)))
    return out


def _pg_arrays(poses, fixed, i, j, Z, w):
    P = _poses_12(poses, "poses")
    N = len(P)
    i, j = np.asarray(i, np.int64).reshape(-1), np.asarray(j, np.int64).reshape(-1)
    E = len(i)
    Z = np.ascontiguousarray(Z, np.float64).reshape(E, 12)
    w = np.ascontiguousarray(w, np.float64).reshape(E, 2)
    fixed = np.asarray(fixed).astype(bool).reshape(-1)
    if fixed.shape != (N,) or j.shape != (E,):
        raise ValueError("fixed must be [%d] and i, j of one length" % N)
    return P, fixed, i, j, Z, w


def pose_graph_linearize(poses, fixed, i, j, Z, w, lam, words=None):
    """One linearisation of a pose graph - the definition of include/stereo_vision_hip.h (AE1) in numpy.  poses float64 [N,12] world
    from frame, fixed bool [N], edges i, j int [E], Z float64 [E,12] the measured P_i^-1 o P_j, w float64 [E,2] = (w_rot, w_trans) as
    they count now (a switched-off edge has both 0), lam > 0.  -> {"M" [E,12], "Wr" [E,6], "chi2" [E], "b" [N,6], "factor" [N,21]}.

      M        P_j^-1 o P_i: R_M[a,b] = (Rj[0,a] Ri[0,b] + Rj[1,a] Ri[1,b]) + Rj[2,a] Ri[2,b]; t_M = Rj^T (t_i - t_j), every three-term sum
               (p0 + p1) + p2.
      residual Q = M o Z (R_Q = R_M R_Z, t_Q = R_M t_Z + t_M), D = Q^-1; a = 0.5 (Q[1,2] - Q[2,1], Q[2,0] - Q[0,2], Q[0,1] - Q[1,0]),
               t_D = -(R_Q^T t_Q); Wr = (w_rot a, w_trans t_D); chi2 = w_rot ((a0 a0 + a1 a1) + a2 a2) + w_trans ((t0 t0 + t1 t1) + t2 t2).
      b        per pose, from 0.0 over its entries in ascending order: - Wr where it is the edge's j, + Ad_M^T Wr where it is its i; 0 for a
               fixed pose.
      block    the 6 x 6 diagonal block of H as 21 words (row p, column q <= p), from 0.0 over the same entries: + diag(w) where the pose
               is j; + A^T W A where it is i, A = Ad_M = [[R, 0], [T, R]], T[a,b] = (t x column b of R)[a], each word the six products (A[m,p]
               w[m]) A[m,q], m = 0 .. 5, added left to right; then + lam on the diagonal.
      factor   its L D L^T, in place: d_p = B[p,p] - sum_q<p (L[p,q] d_q) L[p,q]; L[r,p] = (B[r,p] - sum_q<p (L[r,q] d_q) L[p,q]) / d_p; the
               sums subtracted one by one, q ascending.  d on the diagonal words, L below."""
    P, fixed, i, j, Z, w = _pg_arrays(poses, fixed, i, j, Z, w)
    N, E = len(P), len(i)
    lam = float(lam)
    row_start, inc = pose_graph_words(N, i, j) if words is None else words
    Pi, Pj = P[i], P[j]
    RM = np.stack([(Pj[:, a] * Pi[:, b] + Pj[:, 3 + a] * Pi[:, 3 + b]) + Pj[:, 6 + a] * Pi[:, 6 + b] for a in range(3) for b in range(3)], -1).reshape(E, 9)
    M = np.concatenate([RM, _pg_mtv(Pj[:, :9], Pi[:, 9:] - Pj[:, 9:])], -1).reshape(E, 12)
    RQ = np.stack([(RM[:, 3 * a] * Z[:, b] + RM[:, 3 * a + 1] * Z[:, 3 + b]) + RM[:, 3 * a + 2] * Z[:, 6 + b] for a in range(3) for b in range(3)], -1).reshape(E, 9)
    tQ = _pg_mv(RM, Z[:, 9:]) + M[:, 9:]
    a = np.stack([0.5 * (RQ[:, 5] - RQ[:, 7]), 0.5 * (RQ[:, 6] - RQ[:, 2]), 0.5 * (RQ[:, 1] - RQ[:, 3])], -1).reshape(E, 3)
    tD = -_pg_mtv(RQ, tQ)
    Wr = np.concatenate([w[:, :1] * a, w[:, 1:] * tD], -1).reshape(E, 6)
    chi2 = w[:, 0] * ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]) + w[:, 1] * ((tD[:, 0] * tD[:, 0] + tD[:, 1] * tD[:, 1]) + tD[:, 2] * tD[:, 2])
    # A = Ad_M, [E,6,6], and the edge's own block A^T W A
    A = np.zeros((E, 6, 6))
    R3 = RM.reshape(E, 3, 3)
    A[:, :3, :3] = R3
    A[:, 3:, 3:] = R3
    for c in range(3):
        A[:, 3:, c] = _pg_cross(M[:, 9:], R3[:, :, c])
    w6 = np.concatenate([np.repeat(w[:, :1], 3, 1), np.repeat(w[:, 1:], 3, 1)], 1).reshape(E, 6)
    Be = np.zeros((E, 21))
    for n, (p, q) in enumerate(_PG_TRI):
        s = (A[:, 0, p] * w6[:, 0]) * A[:, 0, q]
        for m in range(1, 6):
            s = s + (A[:, m, p] * w6[:, m]) * A[:, m, q]
        Be[:, n] = s
    up = _pg_adt(M, Wr)
    b, B = np.zeros((N, 6)), np.zeros((N, 21))
    diag = np.array(_PG_DIAG)
    for k, e, is_i in _pg_ranks(row_start, inc):
        b[k] = np.where(is_i[:, None], b[k] + up[e], b[k] - Wr[e])
        B[k[is_i]] = B[k[is_i]] + Be[e[is_i]]
        kj = k[~is_i]
        B[kj[:, None], diag[None, :]] = B[kj[:, None], diag[None, :]] + w6[e[~is_i]]
    b[fixed] = 0.0
    B[:, diag] = B[:, diag] + lam
    F = B.copy()
    at = _PG_AT
    for p in range(6):
        s = F[:, at[(p, p)]]
        for q in range(p):
            s = s - (F[:, at[(p, q)]] * F[:, at[(q, q)]]) * F[:, at[(p, q)]]
        F[:, at[(p, p)]] = s
        for r in range(p + 1, 6):
            s = F[:, at[(r, p)]]
            for q in range(p):
                s = s - (F[:, at[(r, q)]] * F[:, at[(q, q)]]) * F[:, at[(p, q)]]
            F[:, at[(r, p)]] = s / F[:, at[(p, p)]]
    return {"M": M, "Wr": Wr, "chi2": chi2, "b": b, "factor": F}


def _pg_precondition(F, r):
    """z = (L D L^T)^-1 r per pose: forward y_p = r_p - sum_q<p L[p,q] y_q, then y_p / d_p, then backward z_p = y_p - sum_q>p L[q,p] z_q,
    the sums subtracted one by one with q ascending."""
    at = _PG_AT
    y = [None] * 6
    for p in range(6):
        s = r[..., p]
        for q in range(p):
            s = s - F[..., at[(p, q)]] * y[q]
        y[p] = s
    y = [y[p] / F[..., at[(p, p)]] for p in range(6)]
    z = [None] * 6
    for p in range(5, -1, -1):
        s = y[p]
        for q in range(p + 1, 6):
            s = s - F[..., at[(q, p)]] * z[q]
        z[p] = s
    return np.stack(z, -1)


def _pg_operator(x, fixed, i, j, w6, M, ranks, lam):
    """H x in the two passes of the definition: g_e = W (x_j - Ad_M x_i) per edge; per pose, from 0.0 over its entries in ascending order,
    + g_e where it is j and - Ad_M^T g_e where it is i, then + lam x_k; 0 for a fixed pose."""
    g = w6 * (x[j] - _pg_ad(M, x[i]))
    down = _pg_adt(M, g)
    q = np.zeros_like(x)
    for k, e, is_i in ranks:
        q[k] = np.where(is_i[:, None], q[k] - down[e], q[k] + g[e])
    q = q + lam * x
    q[fixed] = 0.0
    return q


def pose_graph_pcg(fixed, i, j, w, M, b, factor, lam, max_iters, tol, words=None):
    """Preconditioned conjugate gradients on H x = b from x = 0 - the definition of include/stereo_vision_hip.h (AE2) in numpy, over what
    pose_graph_linearize gave.  -> x float64 [N,6], {"iteration", "done", "rr", "rr0"}.

      start     r = b, z = F^-1 r per pose (_pg_precondition), rr0 = rr = <r, r>, rz = <r, z>; every <a, b> is pose_graph_sum of the poses'
                six products added left to right.
      verdict   done = rr <= (tol tol) rr0, in double, before the first iteration and after every one; nothing moves once it holds.
      iteration p = z in the first, else z + (rz / rz_before) p; q = H p (_pg_operator); alpha = rz / <p, q>; x = x + alpha p; r = r -
                alpha q; z = F^-1 r; rr = <r, r>; rz = <r, z>."""
    i, j = np.asarray(i, np.int64).reshape(-1), np.asarray(j, np.int64).reshape(-1)
    fixed = np.asarray(fixed).astype(bool).reshape(-1)
    N, E = len(fixed), len(i)
    w = np.asarray(w, np.float64).reshape(E, 2)
    w6 = np.concatenate([np.repeat(w[:, :1], 3, 1), np.repeat(w[:, 1:], 3, 1)], 1).reshape(E, 6)
    M, b, F = np.asarray(M, np.float64).reshape(E, 12), np.asarray(b, np.float64).reshape(N, 6), np.asarray(factor, np.float64).reshape(N, 21)
    lam, tol2 = float(lam), float(tol) * float(tol)
    ranks = _pg_ranks(*(pose_graph_words(N, i, j) if words is None else words))
    x, r = np.zeros((N, 6)), b.copy()
    z = _pg_precondition(F, r)
    p = np.zeros((N, 6))
    rr0 = rr = pose_graph_sum(_pg_dot6(r, r))
    rz, rz_before = pose_graph_sum(_pg_dot6(r, z)), None
    it, done = 0, rr <= tol2 * rr0
    while not done and it < max_iters:
        p = z.copy() if it == 0 else z + (rz / rz_before) * p
        q = _pg_operator(p, fixed, i, j, w6, M, ranks, lam)
        alpha = rz / pose_graph_sum(_pg_dot6(p, q))
        x = x + alpha * p
        r = r - alpha * q
        z = _pg_precondition(F, r)
        rr = pose_graph_sum(_pg_dot6(r, r))
        rz_before, rz = rz, pose_graph_sum(_pg_dot6(r, z))
        it += 1
        done = rr <= tol2 * rr0
    return x, {"iteration": it, "done": bool(done), "rr": float(rr), "rr0": float(rr0)}


def _pgb_mv(R, x):
    return [(R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2] for a in range(3)]


def _pgb_mtv(R, x):
    return [(R[a] * x[0] + R[3 + a] * x[1]) + R[6 + a] * x[2] for a in range(3)]


def _pgb_cross(t, u):
    return [t[1] * u[2] - t[2] * u[1], t[2] * u[0] - t[0] * u[2], t[0] * u[1] - t[1] * u[0]]


def _pgb_ad(M, x):
    u, v = _pgb_mv(M[:9], x[:3]), _pgb_mv(M[:9], x[3:])
    c = _pgb_cross(M[9:], u)
    return u + [c[a] + v[a] for a in range(3)]


def _pgb_adt(M, g):
    c = _pgb_cross(M[9:], g[3:])
    return _pgb_mtv(M[:9], [g[a] - c[a] for a in range(3)]) + _pgb_mtv(M[:9], g[3:])


def _pgb_lists(n_poses, i, j):
    lists = [[] for _ in range(n_poses)]
    for e in range(len(i)):
        lists[j[e]].append((e, False))
        lists[i[e]].append((e, True))
    return lists


def pose_graph_linearize_brute(poses, fixed, i, j, Z, w, lam):
    """pose_graph_linearize as plain loops over edges and poses, in Python floats."""
    P, fixed, i, j, Z, w = _pg_arrays(poses, fixed, i, j, Z, w)
    N, E = len(P), len(i)
    P, Z, w, i, j, lam = P.tolist(), Z.tolist(), w.tolist(), i.tolist(), j.tolist(), float(lam)
    M, Wr, chi2, Be = [], [], [], []
    for e in range(E):
        Pi, Pj, Ze, (wr, wt) = P[i[e]], P[j[e]], Z[e], w[e]
        RM = [(Pj[a] * Pi[b] + Pj[3 + a] * Pi[3 + b]) + Pj[6 + a] * Pi[6 + b] for a in range(3) for b in range(3)]
        tM = _pgb_mtv(Pj[:9], [Pi[9 + a] - Pj[9 + a] for a in range(3)])
        RQ = [(RM[3 * a] * Ze[b] + RM[3 * a + 1] * Ze[3 + b]) + RM[3 * a + 2] * Ze[6 + b] for a in range(3) for b in range(3)]
        u = _pgb_mv(RM, Ze[9:])
        tQ = [u[a] + tM[a] for a in range(3)]
        a = [0.5 * (RQ[5] - RQ[7]), 0.5 * (RQ[6] - RQ[2]), 0.5 * (RQ[1] - RQ[3])]
        tD = [-v for v in _pgb_mtv(RQ, tQ)]
        M.append(RM + tM)
        Wr.append([wr * v for v in a] + [wt * v for v in tD])
        chi2.append(wr * ((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + wt * ((tD[0] * tD[0] + tD[1] * tD[1]) + tD[2] * tD[2]))
        A = [[0.0] * 6 for _ in range(6)]
        for c in range(3):
            T = _pgb_cross(tM, [RM[c], RM[3 + c], RM[6 + c]])
            for a_ in range(3):
                A[a_][c] = RM[3 * a_ + c]
                A[3 + a_][3 + c] = RM[3 * a_ + c]
                A[3 + a_][c] = T[a_]
        w6 = [wr, wr, wr, wt, wt, wt]
        blk = []
        for p, q in _PG_TRI:
            s = (A[0][p] * w6[0]) * A[0][q]
            for m in range(1, 6):
                s = s + (A[m][p] * w6[m]) * A[m][q]
            blk.append(s)
        Be.append(blk)
    b, F = [], []
    for k, entries in enumerate(_pgb_lists(N, i, j)):
        acc, B = [0.0] * 6, [0.0] * 21
        for e, is_i in entries:
            if is_i:
                up = _pgb_adt(M[e], Wr[e])
                acc = [acc[c] + up[c] for c in range(6)]
                B = [B[n] + Be[e][n] for n in range(21)]
            else:
                acc = [acc[c] - Wr[e][c] for c in range(6)]
                for p in range(6):
                    B[_PG_AT[(p, p)]] = B[_PG_AT[(p, p)]] + (w[e][0] if p < 3 else w[e][1])
        for p in range(6):
            B[_PG_AT[(p, p)]] = B[_PG_AT[(p, p)]] + lam
        at = _PG_AT
        for p in range(6):
            s = B[at[(p, p)]]
            for q in range(p):
                s = s - (B[at[(p, q)]] * B[at[(q, q)]]) * B[at[(p, q)]]
            B[at[(p, p)]] = s
            for r in range(p + 1, 6):
                s = B[at[(r, p)]]
                for q in range(p):
                    s = s - (B[at[(r, q)]] * B[at[(q, q)]]) * B[at[(p, q)]]
                B[at[(r, p)]] = s / B[at[(p, p)]]
        b.append([0.0] * 6 if fixed[k] else acc)
        F.append(B)
    f64 = np.float64
    return {"M": np.array(M, f64).reshape(E, 12), "Wr": np.array(Wr, f64).reshape(E, 6), "chi2": np.array(chi2, f64).reshape(E),
            "b": np.array(b, f64).reshape(N, 6), "factor": np.array(F, f64).reshape(N, 21)}


def pose_graph_pcg_brute(fixed, i, j, w, M, b, factor, lam, max_iters, tol):
    """pose_graph_pcg as plain loops over edges and poses, in Python floats."""
    i, j = np.asarray(i, np.int64).reshape(-1).tolist(), np.asarray(j, np.int64).reshape(-1).tolist()
    fixed = np.asarray(fixed).astype(bool).reshape(-1).tolist()
    N, E = len(fixed), len(i)
    w, M = np.asarray(w, np.float64).reshape(E, 2).tolist(), np.asarray(M, np.float64).reshape(E, 12).tolist()
    b, F = np.asarray(b, np.float64).reshape(N, 6).tolist(), np.asarray(factor, np.float64).reshape(N, 21).tolist()
    lam, tol2, at = float(lam), float(tol) * float(tol), _PG_AT
    lists = _pgb_lists(N, i, j)

    def dot(u, v):
        return pose_graph_sum_brute([((((u[k][0] * v[k][0] + u[k][1] * v[k][1]) + u[k][2] * v[k][2]) + u[k][3] * v[k][3]) + u[k][4] * v[k][4])
                                     + u[k][5] * v[k][5] for k in range(N)])

    def precondition(k, r):
        y = []
        for p in range(6):
            s = r[p]
            for q in range(p):
                s = s - F[k][at[(p, q)]] * y[q]
            y.append(s)
        y = [y[p] / F[k][at[(p, p)]] for p in range(6)]
        z = [0.0] * 6
        for p in range(5, -1, -1):
            s = y[p]
            for q in range(p + 1, 6):
                s = s - F[k][at[(q, p)]] * z[q]
            z[p] = s
        return z

    x, r = [[0.0] * 6 for _ in range(N)], [row[:] for row in b]
    z = [precondition(k, r[k]) for k in range(N)]
    p = [[0.0] * 6 for _ in range(N)]
    rr0 = rr = dot(r, r)
    rz, rz_before = dot(r, z), None
    it, done = 0, rr <= tol2 * rr0
    while not done and it < max_iters:
        if it == 0:
            p = [row[:] for row in z]
        else:
            beta = rz / rz_before
            p = [[z[k][c] + beta * p[k][c] for c in range(6)] for k in range(N)]
        g = []
        for e in range(E):
            ad = _pgb_ad(M[e], p[i[e]])
            g.append([(w[e][0] if c < 3 else w[e][1]) * (p[j[e]][c] - ad[c]) for c in range(6)])
        q = []
        for k in range(N):
            acc = [0.0] * 6
            for e, is_i in lists[k]:
                if is_i:
                    down = _pgb_adt(M[e], g[e])
                    acc = [acc[c] - down[c] for c in range(6)]
                else:
                    acc = [acc[c] + g[e][c] for c in range(6)]
            q.append([0.0] * 6 if fixed[k] else [acc[c] + lam * p[k][c] for c in range(6)])
        alpha = rz / dot(p, q)
        x = [[x[k][c] + alpha * p[k][c] for c in range(6)] for k in range(N)]
        r = [[r[k][c] - alpha * q[k][c] for c in range(6)] for k in range(N)]
        z = [precondition(k, r[k]) for k in range(N)]
        rr = dot(r, r)
        rz_before, rz = rz, dot(r, z)
        it += 1
        done = rr <= tol2 * rr0
    return np.array(x, np.float64).reshape(N, 6), {"iteration": it, "done": bool(done), "rr": float(rr), "rr0": float(rr0)}


def pose_between(a, b):
    """a^-1 o b of two [12] poses: the relative pose an edge of the pose graph measures, Z = P_i^-1 o P_j."""
    return _pose_mul(_pose_inv(np.asarray(a, np.float64).reshape(12)), np.asarray(b, np.float64).reshape(12))


def pose_graph_chain(poses, w_rot=1.0, w_trans=1.0):
    """The odometry edges of a chain of poses [N,12]: edge k ties frames k and k + 1 with Z = poses[k]^-1 o poses[k + 1] and the weights
    given (scalars, or [N - 1]).  -> (i, j, Z, w, kind), the edge tuple pose_graph takes."""
    P = _poses_12(poses, "poses")
    n = max(len(P) - 1, 0)
    Z = np.array([_pose_mul(_pose_inv(P[k]), P[k + 1]) for k in range(n)], np.float64).reshape(n, 12)
    w = np.stack([np.broadcast_to(np.asarray(w_rot, np.float64), (n,)), np.broadcast_to(np.asarray(w_trans, np.float64), (n,))], 1).reshape(n, 2)
    return np.arange(n, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32), Z, np.ascontiguousarray(w), np.zeros(n, np.int32)


def pose_graph_loop(i, j, Z, w_rot=1.0, w_trans=1.0):
    """One loop edge: frames i and j with the measured Z = P_i^-1 o P_j [12] - say pose_mul(inverse of key i's pose, the pose
    VoxelMap.align arrived at for frame j) - and its weights.  -> the edge tuple pose_graph takes."""
    Z = np.asarray(Z, np.float64)
    if Z.shape != (12,):
        raise ValueError("Z must be float64 [12], got shape %s" % (Z.shape,))
    return (np.array([_whole(i, "i")], np.int32), np.array([_whole(j, "j")], np.int32), Z.reshape(1, 12).copy(),
            np.array([[float(w_rot), float(w_trans)]], np.float64), np.ones(1, np.int32))


def pose_graph(poses, edges, fixed=(0,)):
    """A pose graph, checked: poses float64 [N,12] (world from frame, N in 1 .. 2^20), edges a list of edge tuples (pose_graph_chain's,
    pose_graph_loop's) joined in the order given (at most 2^22), fixed the indices of the poses held (or a bool mask [N]).  -> {"poses",
    "i", "j", "Z", "w", "kind", "fixed"}.  ValueError for i == j, an index outside 0 .. N - 1, a weight that is negative or not finite,
    poses or Z that are not finite, a kind that is neither 0 nor 1, and no fixed pose."""
    P = _poses_12(poses, "poses").copy()
    N = len(P)
    if not 1 <= N <= POSE_GRAPH_POSES_MAX:
        raise ValueError("a pose graph holds 1 .. 2^20 poses, got %d" % N)
    if not np.isfinite(P).all():
        raise ValueError("a pose is not finite")
    parts = [tuple(np.asarray(a) for a in t) for t in edges]
    for t in parts:
        if len(t) != 5 or not (len(t[0]) == len(t[1]) == len(t[2]) == len(t[3]) == len(t[4])) or t[2].shape[1:] != (12,) or t[3].shape[1:] != (2,):
            raise ValueError("an edge tuple is (i [E], j [E], Z [E,12], w [E,2], kind [E])")
    cat = lambda n, dt, shape: (np.concatenate([t[n].astype(dt) for t in parts]) if parts else np.zeros((0,) + shape, dt)).reshape((-1,) + shape)
    i, j, Z, w, kind = cat(0, np.int64, ()), cat(1, np.int64, ()), cat(2, np.float64, (12,)), cat(3, np.float64, (2,)), cat(4, np.int64, ())
    if len(i) > POSE_GRAPH_EDGES_MAX:
        raise ValueError("a pose graph holds at most 2^22 edges, got %d" % len(i))
    if ((i < 0) | (i >= N) | (j < 0) | (j >= N)).any():
        raise ValueError("an edge names a pose outside 0 .. %d" % (N - 1))
    if (i == j).any():
        raise ValueError("an edge ties a pose to itself")
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("a weight is negative or not finite")
    if not np.isfinite(Z).all():
        raise ValueError("a measurement Z is not finite")
    if ((kind != POSE_GRAPH_ODOMETRY) & (kind != POSE_GRAPH_LOOP)).any():
        raise ValueError("a kind is neither 0 (odometry) nor 1 (loop)")
    f = np.asarray(fixed)
    if f.dtype == bool:
        if f.shape != (N,):
            raise ValueError("a fixed mask must be [%d]" % N)
        mask = f.copy()
    else:
        f = f.astype(np.int64).reshape(-1)
        if ((f < 0) | (f >= N)).any():
            raise ValueError("a fixed pose lies outside 0 .. %d" % (N - 1))
        mask = np.zeros(N, bool)
        mask[f] = True
    if not mask.any():
        raise ValueError("a pose graph needs a fixed pose: without one the whole trajectory floats")
    return {"poses": P, "i": i.astype(np.int32), "j": j.astype(np.int32), "Z": np.ascontiguousarray(Z), "w": np.ascontiguousarray(w),
            "kind": kind.astype(np.int32), "fixed": mask}


def pose_graph_step(graph, poses, w, lam, max_iters, tol, words):
    """One round's linearise and solve in numpy -> (delta [N,6], chi2 [E], PCG's state): what pose_graph_optimize calls where no device
    step is given."""
    lin = pose_graph_linearize(poses, graph["fixed"], graph["i"], graph["j"], graph["Z"], w, lam, words)
    x, state = pose_graph_pcg(graph["fixed"], graph["i"], graph["j"], w, lin["M"], lin["b"], lin["factor"], lam, max_iters, tol, words)
    return x, lin["chi2"], state


def pose_graph_optimize(graph, rounds=10, gate=None, eps=1e-9, lam=1e-6, max_iters=None, tol=1e-8, step=None):
    """Gauss-Newton on a pose graph (pose_graph's dict): per round linearise and solve (step: pose_graph_step, or the device's with the
    same signature), then on the host P_k <- P_k o pose_exp(delta_k), then every loop edge whose chi2 - at this round's linearisation -
    exceeds `gate` is switched off for the rounds after (odometry edges never; gate=None gates nothing).  Stops after `rounds`, or when
    max |delta| < eps.  max_iters caps PCG per round; None is max(1000, 20 N) - block-Jacobi needs 6 to 12 N iterations on a chain with
    few loops, and a round that stops at the cap is an inexact Gauss-Newton step: "converged" says which did.  -> poses [N,12], {"costs": the sum of chi2 (pose_graph_sum) at each round's linearisation, "cost": the same at the
    poses returned, "iterations": PCG's per round, "converged": PCG's verdicts, "off": the loop edges switched off, ascending, "rounds"}.
    Host code shared by the CPU and the GPU path: the same delta gives the same poses bit for bit."""
    lam, tol = float(lam), float(tol)
    if not (lam > 0.0 and np.isfinite(lam)):
        raise ValueError("lam must be a finite number > 0: it keeps a pose without a live edge solvable")
    if not (tol >= 0.0) or not np.isfinite(tol):
        raise ValueError("tol must be finite and not negative")
    rounds, max_iters = _whole(rounds, "rounds"), _whole(max(1000, 20 * len(graph["poses"])) if max_iters is None else max_iters, "max_iters")
    if rounds < 0 or max_iters < 0:
        raise ValueError("rounds and max_iters must not be negative")
    if gate is not None and not float(gate) >= 0.0:
        raise ValueError("gate must be None or a number >= 0")
    step = pose_graph_step if step is None else step
    P = graph["poses"].copy()
    N = len(P)
    words = pose_graph_words(N, graph["i"], graph["j"])
    live = np.ones(len(graph["i"]), bool)
    is_loop = graph["kind"] == POSE_GRAPH_LOOP
    costs, iterations, converged, done_rounds = [], [], [], 0
    for _ in range(rounds):
        w = graph["w"] * live[:, None]
        delta, chi2, state = step(graph, P, w, lam, max_iters, tol, words)
        costs.append(pose_graph_sum(chi2))
        iterations.append(int(state["iteration"]))
        converged.append(bool(state["done"]))
        for k in range(N):
            if not graph["fixed"][k]:
                P[k] = _pose_mul(P[k], pose_exp(delta[k]))
        done_rounds += 1
        if gate is not None:
            live &= ~(is_loop & (chi2 > float(gate)))
        if not np.abs(delta).max() >= eps:
            break
    w = graph["w"] * live[:, None]
    cost = pose_graph_sum(pose_graph_linearize(P, graph["fixed"], graph["i"], graph["j"], graph["Z"], w, lam, words)["chi2"])
    return P, {"costs": costs, "cost": cost, "iterations": iterations, "converged": converged, "off": np.nonzero(is_loop & ~live)[0].astype(np.int32),
               "rounds": done_rounds}


VOXEL_CARVE_REACH_MAX = 1023  # cells a ray of voxel_map_carve may span on its major axis: 2 k d + nst stays below 2^22
VOXEL_CARVE_MARGIN_MAX = 255
VOXEL_CARVE_STATS = ("rays", "steps", "touched", "carved")  # voxel_map_carve's counts, in the order of the C entry's stats


def voxel_map_carve(map_state, xyz, n, counts, poses, origin=(0.0, 0.0, 0.0), seq0=0, reach=VOXEL_CARVE_REACH_MAX, margin=1, min_miss=1, ratio=0, apply=True):
    """Carves free space out of a voxel map along the sight lines of B frames: the definition of include/stereo_vision_hip.h (T) in numpy.
    map_state (voxel_map_state's dict) is changed in place under `apply`; xyz, n, counts, poses and seq0 are voxel_map_insert's - the usual
    call repeats the insert's own arguments, behind the insert.  -> {"rays", "steps", "touched", "carved": ints, "key": int64 [T] - the
    touched voxels, ascending -, "miss": int64 [T] - theirs}.

      sensor   O[k] = ((R[k,0] ox + R[k,1] oy) + R[k,2] oz) + t[k] with origin = (ox, oy, oz), the sensor's centre in the frame's axes:
               the insert's expression.  Frame b casts rays iff its twelve pose words are finite and lo < O < hi strictly; c0 is O's cell
               by the insert's rule, min(int((O - lo) / size), cells - 1).
      rows     the insert's: the first min(counts[b], cap), kept iff w > 0 and lo < Pw < hi strictly; c1 is the row's cell.
      ray      d = c1 - c0, nst = max |d_a|; a kept row of a casting frame casts a ray iff nst <= reach (1 .. 1023 cells) - "rays".  Its
               steps k = 1 .. nst - 1 - margin (margin 0 .. 255 cells in front of the row's own cell are left alone; there may be no
               step) - "steps" - lie in the cells c0_a + (2 k d_a + nst) // (2 nst): occupancy_ray_cells' rule per axis, flooring.
      miss     a step whose cell holds a voxel with last_seq < seq0 + b adds the row's weight to that voxel's miss: a voxel this frame
               or a later one has seen is never counted against.  (An emptied voxel reads as last_seq 0, the word the table holds.)
               miss starts from zero in every call.  Contract: miss < 2^47 per voxel.
      verdict  "touched": the voxels with miss > 0.  "carved": those with miss >= min_miss (>= 1) and 256 miss >= ratio n (ratio 0 ..
               65535, in 1 / 256 of the voxel's own weight n).
      apply    a carved voxel keeps its row - its key - with n = S = C = m = 0 and the first_seq / last_seq an insert starts a voxel
               from: the tombstone of the device's table.  A later insert or carry adds to it as to a fresh voxel, every call skips it
               at min_n >= 1 - the defaults -, and a carry (a prune) drops it as "filtered".  Until then voxel_map_rows is defined for
               min_n >= 1 only: n = 0 divides.  The number of voxels the map holds does not change.
    An overflowed map: nothing is done, rays is -1 and the other counts 0.  ValueError for a bad argument."""
    w = map_state["params"]
    lo, hi, size, cells = np.array(w["lo"]), np.array(w["hi"]), np.float64(w["size"]), np.array(w["cells"], np.int64)
    xyz = np.asarray(xyz)
    if xyz.dtype not in (np.float32, np.float64) or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be float32 or float64 [B,cap,3], got %s %s" % (xyz.dtype, xyz.shape))
    B, cap = xyz.shape[:2]
    counts = np.asarray(counts)
    poses = np.asarray(poses, np.float64)
    if counts.shape != (B,) or poses.shape != (B, 12):
        raise ValueError("counts must be [B] and poses [B,12] for B = %d, got %s and %s" % (B, counts.shape, poses.shape))
    if n is not None and np.asarray(n).shape != (B, cap):
        raise ValueError("n must be [B,cap] or None")
    if B > VOXEL_MATCH_BATCH_MAX:
        raise ValueError("at most 65535 frames per call, got %d" % B)
    try:
        origin = np.array([float(v) for v in origin], np.float64)
    except (TypeError, ValueError):
        origin = np.zeros(0)
    if origin.shape != (3,) or not np.isfinite(origin).all():
        raise ValueError("origin must be three finite numbers")
    seq0, reach, margin = _whole(seq0, "seq0"), _whole(reach, "reach"), _whole(margin, "margin")
    min_miss, ratio = _whole(min_miss, "min_miss"), _whole(ratio, "ratio")
    if seq0 < 0 or seq0 + B - 1 > VOXEL_MAP_SEQ_MAX:
        raise ValueError("the sequence numbers seq0 .. seq0 + B - 1 must stay in 0 .. 2^31 - 2, got seq0 = %r" % (seq0,))
    if not 1 <= reach <= VOXEL_CARVE_REACH_MAX or not 0 <= margin <= VOXEL_CARVE_MARGIN_MAX:
        raise ValueError("reach must be in 1 .. %d and margin in 0 .. %d, got %d and %d" % (VOXEL_CARVE_REACH_MAX, VOXEL_CARVE_MARGIN_MAX, reach, margin))
    if not 1 <= min_miss < 2 ** 63 or not 0 <= ratio <= 65535:
        raise ValueError("min_miss must be an int64 >= 1 and ratio in 0 .. 65535, got %d and %d" % (min_miss, ratio))
    if apply not in (0, 1):
        raise ValueError("apply must be 0 or 1, got %r" % (apply,))
    out = dict.fromkeys(VOXEL_CARVE_STATS, 0)
    out.update(key=np.zeros(0, np.int64), miss=np.zeros(0, np.int64))
    if map_state["overflowed"]:
        out["rays"] = -1
        return out
    rows = np.arange(cap)[None, :] < np.minimum(counts.astype(np.int64), cap)[:, None]  # [B,cap]: the rows a frame has
    R = poses[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):  # rows beyond counts, and poses that cast nothing, may hold anything
        ox, oy, oz = origin
        O = np.stack([((poses[:, 3 * k] * ox + poses[:, 3 * k + 1] * oy) + poses[:, 3 * k + 2] * oz) + poses[:, 9 + k] for k in range(3)], -1)  # [B,3]
        casts = np.isfinite(poses).all(1) & ((lo < O) & (O < hi)).all(-1)
        P = xyz.astype(np.float64)
        x, y, z = P[..., 0], P[..., 1], P[..., 2]
        Pw = np.stack([((R[..., 3 * k] * x + R[..., 3 * k + 1] * y) + R[..., 3 * k + 2] * z) + R[..., 9 + k] for k in range(3)], -1)
        inside = ((lo < Pw) & (Pw < hi)).all(-1)
    wt = np.ones((B, cap), np.int64) if n is None else np.asarray(n).astype(np.int64)
    keep = rows & inside & (wt > 0) & casts[:, None]
    b_of = np.broadcast_to(np.arange(B, dtype=np.int64)[:, None], (B, cap))[keep]
    c0 = np.minimum(((np.where(casts[:, None], O, lo) - lo) / size).astype(np.int64), cells - 1)[b_of]  # [rows kept, 3]
    c1 = np.minimum(((Pw[keep] - lo) / size).astype(np.int64), cells - 1)
    d = c1 - c0
    nst = np.abs(d).max(-1) if len(d) else np.zeros(0, np.int64)
    ray = nst <= reach
    c0, d, nst, wk, seq = c0[ray], d[ray], nst[ray], wt[keep][ray], seq0 + b_of[ray]
    ns = np.maximum(nst - 1 - margin, 0)
    out["rays"], out["steps"] = int(ray.sum()), int(ns.sum())
    by_key = np.argsort(map_state["key"], kind="stable")
    vkey = map_state["key"][by_key]
    vlast = np.maximum(map_state["last_seq"][by_key], 0)  # what the table holds for a voxel that was emptied
    miss = np.zeros(len(vkey), np.int64)
    for k in range(1, int(ns.max()) + 1 if len(ns) and len(vkey) else 1):
        on = ns >= k  # nst >= 2 there
        den = 2 * nst[on][:, None]
        c = c0[on] + (2 * k * d[on] + nst[on][:, None]) // den
        key = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
        at = np.minimum(np.searchsorted(vkey, key), len(vkey) - 1)
        hit = (vkey[at] == key) & (vlast[at] < seq[on])
        np.add.at(miss, at[hit], wk[on][hit])
    touched = miss > 0
    carved = touched & (miss >= min_miss) & (256 * miss >= ratio * map_state["n"][by_key])
    out["touched"], out["carved"] = int(touched.sum()), int(carved.sum())
    out["key"], out["miss"] = vkey[touched], miss[touched]
    if apply:
        gone = by_key[carved]
        for f in ("n", "S", "C", "m"):
            map_state[f][gone] = 0
        map_state["first_seq"][gone], map_state["last_seq"][gone] = np.iinfo(np.int64).max, -1
    return out


VOXEL_RENDER_VIEWS_MAX = 4096
VOXEL_RENDER_SIDE_MAX = 8192    # width and height of a rendered image at most
VOXEL_RENDER_R_MAX = 8          # r_max at most: a voxel covers at most 17 x 17 pixels
VOXEL_RENDER_FAR_MAX = 2.0 ** 20  # cells: zq = int(tz * 256) stays below 2^28
VOXEL_RENDER_LABELS = ("none", "measured", "expected", "agree", "nearer", "farther")  # voxel_map_render's label, 0 .. 5
VOXEL_RENDER_PNG = np.array([[0, 0, 0], [96, 96, 96], [40, 60, 140], [40, 160, 40], [230, 60, 40], [60, 120, 250]], np.uint8)  # --voxel-render: RGB per label
_VOXEL_RENDER_LIM = 2.0 ** 30  # |u|, |v| of a voxel that is kept stay below it


def voxel_render_camera(Q, width, height, size, footprint=1.0):
    """The camera voxel_map_render draws into, from the rig's Q (4x4, the rectified form compact_cloud reprojects with: rows (1, 0, 0, -cx),
    (0, 1, 0, -cy), (0, 0, 0, f), (0, 0, q32, q33)) as a dict: f = Q[2,3], cx = -Q[0,3], cy = -Q[1,3], q32 = Q[3,2], q33 = Q[3,3], width,
    height, size and half_px = (0.5 * footprint) * f - half the edge in pixels, at a depth of one cell, of a square `footprint` voxels
    wide (a voxel of `size` metres at tz cells spans f * size / (tz * size) pixels: the size cancels, and is only checked and kept).
    ValueError for a Q of another form, f <= 0, q32 == 0 or a word that is not finite."""
    Q = np.asarray(Q, np.float64)
    if Q.size != 16:
        raise ValueError("Q must be 4x4, got shape %s" % (Q.shape,))
    Q = Q.reshape(4, 4)
    zeros = [Q[0, 1], Q[0, 2], Q[1, 0], Q[1, 2], Q[2, 0], Q[2, 1], Q[2, 2], Q[3, 0], Q[3, 1]]
    if not (np.isfinite(Q).all() and Q[0, 0] == 1.0 and Q[1, 1] == 1.0 and all(v == 0.0 for v in zeros) and Q[2, 3] > 0.0 and Q[3, 2] != 0.0):
        raise ValueError("Q is not of the rectified form (1 0 0 -cx; 0 1 0 -cy; 0 0 0 f; 0 0 q32 q33) with f > 0 and q32 != 0")
    size, footprint = np.float64(size), np.float64(footprint)
    if not (np.isfinite(size) and size > 0 and np.isfinite(footprint) and footprint >= 0):
        raise ValueError("size must be finite and > 0 and footprint finite and >= 0, got %r and %r" % (size, footprint))
    cam = {"f": float(Q[2, 3]), "cx": float(-Q[0, 3]), "cy": float(-Q[1, 3]), "q32": float(Q[3, 2]), "q33": float(Q[3, 3]), "width": width, "height": height,
           "size": float(size), "half_px": float((np.float64(0.5) * footprint) * Q[2, 3])}
    voxel_render_words(cam)
    return cam


def voxel_render_words(camera, r_max=4, near=None, far=None):
    """The words of sv_voxel_render_spec as a dict - f, cx, cy, q32, q33, half_px, near, far (floats), width, height, r_max (ints) - from a
    camera dict (voxel_render_camera's) and a call's r_max, near and far (cells; None: 1 and 2^20), after the checks the C entry makes
    (ValueError): every float finite, f > 0, q32 != 0, half_px >= 0, width and height in 1 .. 8192, r_max in 0 .. 8, 0 < near < far <= 2^20."""
    try:
        w = {k: float(camera[k]) for k in ("f", "cx", "cy", "q32", "q33", "half_px")}
        w["near"], w["far"] = 1.0 if near is None else float(near), VOXEL_RENDER_FAR_MAX if far is None else float(far)
    except (KeyError, TypeError, ValueError):
        raise ValueError("a camera needs the numbers f, cx, cy, q32, q33 and half_px, and near and far must be numbers")
    if not all(np.isfinite(v) for v in w.values()) or not w["f"] > 0 or w["q32"] == 0 or w["half_px"] < 0:
        raise ValueError("the camera's words must be finite with f > 0, q32 != 0 and half_px >= 0, got %r" % (w,))
    if not 0 < w["near"] < w["far"] <= VOXEL_RENDER_FAR_MAX:
        raise ValueError("near and far need 0 < near < far <= 2^20 cells, got %r and %r" % (near, far))
    for k, v, lo, hi in (("width", camera.get("width"), 1, VOXEL_RENDER_SIDE_MAX), ("height", camera.get("height"), 1, VOXEL_RENDER_SIDE_MAX), ("r_max", r_max, 0, VOXEL_RENDER_R_MAX)):
        if v is None or isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (k, lo, hi, v))
        w[k] = int(v)
    return w


def voxel_render_cams(poses, XR=None, XT=None):
    """float64 [V,12], world to camera (R row-major, then t, voxel_map_pose's layout) - what voxel_map_render takes -, from the poses
    update() inserts frames at ([V,12], or the occupancy map's [V,4]: frame to world, Pw = R Pf + t) and the rig's transform (camera to
    frame, Pf = XR Pc + XT; None: the identity, zero).  R and XR must be rotations: the inverse is the transpose.  On the host, in
    double, every product and sum on its own and in this order: M[i,j] = (R[i,0] XR[0,j] + R[i,1] XR[1,j]) + R[i,2] XR[2,j];
    o[i] = ((R[i,0] XT[0] + R[i,1] XT[1]) + R[i,2] XT[2]) + t[i], the camera's centre in the world; then Rc = M transposed and
    tc[k] = -((Rc[k,0] o[0] + Rc[k,1] o[1]) + Rc[k,2] o[2]), so that Pc = Rc Pw + tc."""
    p = voxel_map_pose_words(poses)
    R, t = p[:, :9].reshape(-1, 3, 3), p[:, 9:]
    XR = np.eye(3) if XR is None else np.asarray(XR, np.float64).reshape(3, 3)
    XT = np.zeros(3) if XT is None else np.asarray(XT, np.float64).reshape(3)
    M = np.stack([np.stack([(R[:, i, 0] * XR[0, j] + R[:, i, 1] * XR[1, j]) + R[:, i, 2] * XR[2, j] for j in range(3)], -1) for i in range(3)], 1)
    o = np.stack([((R[:, i, 0] * XT[0] + R[:, i, 1] * XT[1]) + R[:, i, 2] * XT[2]) + t[:, i] for i in range(3)], -1)
    Rc = M.transpose(0, 2, 1)
    tc = np.stack([-((Rc[:, k, 0] * o[:, 0] + Rc[:, k, 1] * o[:, 1]) + Rc[:, k, 2] * o[:, 2]) for k in range(3)], -1)
    return np.ascontiguousarray(np.concatenate([Rc.reshape(-1, 9), tc], 1))


def _voxel_render_setup(map_state, cams, camera, measured, tol, near, far, r_max, min_n, min_rows, since):
    """What voxel_map_render and voxel_map_render_brute share: the checked arguments, the indices of the voxels that pass the filters
    (none for an overflowed map) and the outputs, every pixel without a winner."""
    w = voxel_render_words(camera, r_max, near, far)
    cams = np.asarray(cams, np.float64)
    if cams.ndim != 2 or cams.shape[1] != 12 or len(cams) > VOXEL_RENDER_VIEWS_MAX or len(cams) * w["width"] * w["height"] >= 2 ** 31:
        raise ValueError("cams must be [V,12] with V <= 4096 and V * width * height < 2^31, got shape %s" % (cams.shape,))
    if isinstance(min_n, bool) or int(min_n) != min_n or min_n < 1:
        raise ValueError("min_n must be an integer >= 1 - a carved voxel has n = 0 and divides -, got %r" % (min_n,))
    V, H, W = len(cams), w["height"], w["width"]
    out = {"depth": np.full((V, H, W), -1, np.int32), "key": np.full((V, H, W), -1, np.int64), "color": np.zeros((V, H, W, 4), np.uint8),
           "disparity": np.full((V, H, W), -1, np.float32), "stats": np.zeros((V, 2), np.int64), "label": None, "counts": None}
    if measured is not None:
        measured = np.asarray(measured)
        if measured.dtype != np.float32 or measured.shape != (V, H, W):
            raise ValueError("measured must be float32 [%d,%d,%d], got %s %s" % (V, H, W, measured.dtype, measured.shape))
        if not tol >= 0:
            raise ValueError("tol must be a number >= 0, got %r" % (tol,))
        out["label"], out["counts"] = np.zeros((V, H, W), np.uint8), np.zeros((V, 6), np.int64)
    if map_state["overflowed"]:
        out["stats"][:, 0] = -1
        sel = np.zeros(0, np.int64)
    else:
        sel = np.flatnonzero((map_state["n"] >= min_n) & (map_state["m"] >= min_rows) & (map_state["last_seq"] >= since))
    return w, cams, measured, sel, out


def voxel_map_render(map_state, cams, camera, measured=None, tol=1.0, near=None, far=None, r_max=4, min_n=1, min_rows=1, since=0):
    """A voxel map rendered into V views of one camera, the definition of include/stereo_vision_hip.h (U) in numpy: what the camera should
    see from each pose if the map is right.  The map is only read.

    cams float64 [V,12]: world to camera, R row-major then t (voxel_render_cams); camera: voxel_render_camera's dict; near < far in cells
    (None: 1 and 2^20); r_max 0 .. 8; min_n >= 1, min_rows, since: voxel_map_rows' filters.  Camera axes are Q's: x right, y down, z
    forward.  Every product, sum and quotient is a double, rounded on its own, in the order written.  Per view and voxel that passes
    the filters: the centre Pw = lo + (c + (S + 0.5 n) / (65536 n)) * size (voxel_map_rows' xyz); Pc[k] = ((R[k,0] Pw.x + R[k,1] Pw.y) +
    R[k,2] Pw.z) + t[k]; tz = Pc[2] / size, kept iff near <= tz < far, zq = int(tz * 256.0); u = (f * Pc[0]) / Pc[2] + cx, v = (f * Pc[1])
    / Pc[2] + cy, kept iff both lie strictly inside -2^30 .. 2^30, px = floor(u + 0.5), py = floor(v + 0.5); r = r_max where half_px / tz
    >= r_max, else int(half_px / tz).  The voxel covers the pixels px - r .. px + r by py - r .. py + r, clipped to the image; one that
    covers a pixel counts into drawn.  The winner of a pixel is the covering voxel with the smallest zq, then the smallest key.
    Returns a dict: depth int32 [V,H,W] = zq (-1 without a winner), key int64 [V,H,W] (-1), color uint8 [V,H,W,4] = the winner's
    (2 C + n) // (2 n) (0), disparity float32 [V,H,W] = float32(e) with z = ((zq + 0.5) / 256.0) * size and e = (f / z - q33) / q32
    (-1), stats int64 [V,2] = drawn, covered - the pixels with a winner; (-1, 0) and no winner anywhere for an overflowed map.
    With measured (float32 [V,H,W], valid where finite and > 0; d = the float widened) also label uint8 [V,H,W] - 0 neither measured
    nor expected, 1 measured only, 2 expected only, 3 |d - e| <= tol, 4 d - e > tol (nearer: something new), 5 d - e < -tol (farther: the
    voxel was seen through) - and counts int64 [V,6], the pixels per label; both None without."""
    w, cams, measured, sel, out = _voxel_render_setup(map_state, cams, camera, measured, tol, near, far, r_max, min_n, min_rows, since)
    V, H, W, rm = len(cams), w["height"], w["width"], w["r_max"]
    p = map_state["params"]
    size = np.float64(p["size"])
    key, n, C = map_state["key"][sel], map_state["n"][sel], map_state["C"][sel]
    c = np.stack([key & 0xFFFFF, (key >> 20) & 0xFFFFF, (key >> 40) & 0xFFFFF], -1)
    nf = n.astype(np.float64)[:, None]
    Pw = np.array(p["lo"]) + (c.astype(np.float64) + (map_state["S"][sel].astype(np.float64) + 0.5 * nf) / (65536.0 * nf)) * size
    f, cx, cy = (np.float64(w[k]) for k in ("f", "cx", "cy"))
    for v in range(V):
        R = cams[v]
        with np.errstate(all="ignore"):
            Pc = [((R[3 * k] * Pw[:, 0] + R[3 * k + 1] * Pw[:, 1]) + R[3 * k + 2] * Pw[:, 2]) + R[9 + k] for k in range(3)]
            tz = Pc[2] / size
            uu, vv = (f * Pc[0]) / Pc[2] + cx, (f * Pc[1]) / Pc[2] + cy
            keep = (w["near"] <= tz) & (tz < w["far"]) & (-_VOXEL_RENDER_LIM < uu) & (uu < _VOXEL_RENDER_LIM) & (-_VOXEL_RENDER_LIM < vv) & (vv < _VOXEL_RENDER_LIM)
            at = np.flatnonzero(keep)
            zq = (tz[at] * 256.0).astype(np.int64)
            px, py = np.floor(uu[at] + 0.5).astype(np.int64), np.floor(vv[at] + 0.5).astype(np.int64)
            q = np.float64(w["half_px"]) / tz[at]
            r = np.where(q >= rm, rm, np.minimum(q, rm).astype(np.int64))
        drawn = (np.maximum(px - r, 0) <= np.minimum(px + r, W - 1)) & (np.maximum(py - r, 0) <= np.minimum(py + r, H - 1))
        out["stats"][v, 0] += int(drawn.sum())
        at, zq, px, py, r = at[drawn], zq[drawn], px[drawn], py[drawn], r[drawn]
        if len(at):
            d = np.arange(-int(r.max()), int(r.max()) + 1)
            X, Y = np.broadcast_arrays(px[:, None, None] + d[None, None, :], py[:, None, None] + d[None, :, None])
            ok = (np.abs(d)[None, None, :] <= r[:, None, None]) & (np.abs(d)[None, :, None] <= r[:, None, None]) & (0 <= X) & (X < W) & (0 <= Y) & (Y < H)
            who = np.broadcast_to(np.arange(len(at))[:, None, None], ok.shape)[ok]
            pix = (Y * W + X)[ok]
            order = np.lexsort((key[at][who], zq[who], pix))  # by pixel, then zq, then key
            first = np.ones(len(order), bool)
            first[1:] = pix[order][1:] != pix[order][:-1]
            win, pix = who[order[first]], pix[order[first]]
            nw = n[at[win]]
            out["depth"][v].reshape(-1)[pix] = zq[win]
            out["key"][v].reshape(-1)[pix] = key[at[win]]
            out["color"][v].reshape(-1, 4)[pix] = ((2 * C[at[win]] + nw[:, None]) // (2 * nw[:, None])).astype(np.uint8)
    has = out["depth"] >= 0
    out["stats"][:, 1] = has.sum((1, 2))
    with np.errstate(all="ignore"):
        z = ((out["depth"].astype(np.float64) + 0.5) / 256.0) * size
        e = (f / z - np.float64(w["q33"])) / np.float64(w["q32"])
        out["disparity"][has] = e[has].astype(np.float32)
        if measured is not None:
            valid = np.isfinite(measured) & (measured > 0)
            diff = measured.astype(np.float64) - e
            both = np.where(diff > tol, 4, np.where(diff < -tol, 5, 3))
            out["label"][...] = np.where(valid & has, both, valid * 1 + has * 2).astype(np.uint8)
            out["counts"][...] = np.stack([(out["label"] == k).sum((1, 2)) for k in range(6)], -1)
    return out


def voxel_map_render_brute(map_state, cams, camera, measured=None, tol=1.0, near=None, far=None, r_max=4, min_n=1, min_rows=1, since=0):
    """voxel_map_render's definition as a plain loop over views, voxels and pixels on Python floats and ints: the form the vectorised one
    is checked against.  Same arguments, same dict."""
    import math
    w, cams, measured, sel, out = _voxel_render_setup(map_state, cams, camera, measured, tol, near, far, r_max, min_n, min_rows, since)
    V, H, W, rm = len(cams), w["height"], w["width"], w["r_max"]
    p = map_state["params"]
    lo, size = [float(x) for x in p["lo"]], float(p["size"])
    best = {}  # (view, y, x) -> (zq, key, voxel)
    for v in range(V):
        R = [float(x) for x in cams[v]]
        for i in sel:
            key, n = int(map_state["key"][i]), int(map_state["n"][i])
            Pw = [lo[k] + (float((key >> (20 * k)) & 0xFFFFF) + (float(int(map_state["S"][i, k])) + 0.5 * float(n)) / (65536.0 * float(n))) * size for k in range(3)]
            Pc = [((R[3 * k] * Pw[0] + R[3 * k + 1] * Pw[1]) + R[3 * k + 2] * Pw[2]) + R[9 + k] for k in range(3)]
            tz = Pc[2] / size
            if not (w["near"] <= tz and tz < w["far"]):
                continue
            zq = int(tz * 256.0)
            uu, vv = (w["f"] * Pc[0]) / Pc[2] + w["cx"], (w["f"] * Pc[1]) / Pc[2] + w["cy"]
            if not (-_VOXEL_RENDER_LIM < uu < _VOXEL_RENDER_LIM and -_VOXEL_RENDER_LIM < vv < _VOXEL_RENDER_LIM):
                continue
            px, py = math.floor(uu + 0.5), math.floor(vv + 0.5)
            q = w["half_px"] / tz
            r = rm if q >= rm else int(q)
            covers = False
            for y in range(max(py - r, 0), min(py + r, H - 1) + 1):
                for x in range(max(px - r, 0), min(px + r, W - 1) + 1):
                    covers = True
                    if (v, y, x) not in best or (zq, key) < best[v, y, x][:2]:
                        best[v, y, x] = (zq, key, i)
            out["stats"][v, 0] += 1 if covers else 0
    for (v, y, x), (zq, key, i) in best.items():
        n = int(map_state["n"][i])
        out["depth"][v, y, x], out["key"][v, y, x] = zq, key
        out["color"][v, y, x] = [(2 * int(map_state["C"][i, j]) + n) // (2 * n) for j in range(4)]
        out["stats"][v, 1] += 1
    with np.errstate(over="ignore"):
        for v in range(V):
            for y in range(H):
                for x in range(W):
                    has, e = (v, y, x) in best, 0.0
                    if has:
                        z = ((float(best[v, y, x][0]) + 0.5) / 256.0) * size
                        e = (w["f"] / z - w["q33"]) / w["q32"]
                        out["disparity"][v, y, x] = np.float32(e)
                    if measured is None:
                        continue
                    d = float(measured[v, y, x])
                    valid = math.isfinite(d) and d > 0
                    lab = (4 if d - e > tol else 5 if d - e < -tol else 3) if valid and has else (1 if valid else 0) + (2 if has else 0)
                    out["label"][v, y, x] = lab
                    out["counts"][v, lab] += 1
    return out


VOXEL_FLATTEN_WORDS = ("mode", "z_ref_q", "step_q", "height_q", "radius", "min_obstacle", "min_ground")  # sv_voxel_flatten_spec, in its order
VOXEL_FLATTEN_STATS = ("drawn", "outside", "below", "ground", "obstacle", "overhead", "occupied_cells", "free_cells")  # voxel_map_flatten's stats
VOXEL_FLATTEN_RADIUS_MAX = 8        # flat cells: the window of the local floor is at most 17 x 17
VOXEL_FLATTEN_CELLS_MAX = 8000000   # rows * cols of the flat map at most: what cost_to_goal and the frontiers take
VOXEL_FLATTEN_ZQ_MAX = 2 ** 28      # a voxel's zq stays below it; step_q < height_q < it
VOXEL_FLATTEN_REF_MAX = 2 ** 30     # |z_ref_q| stays below it, so zq - z_ref_q is an int32
_VOXEL_FLATTEN_NONE = 2 ** 31 - 1   # the minimum over no voxel


def voxel_flatten_words(spec):
    """The words of sv_voxel_flatten_spec as a dict of ints - mode, z_ref_q, step_q, height_q, radius, min_obstacle, min_ground - from a
    dict of them (voxel_flatten_params'; a "reserved" entry must hold zeros only), after the checks the C entry makes (ValueError): mode 0
    or 1, |z_ref_q| < 2^30, 1 <= step_q < height_q < 2^28, radius in 0 .. 8, min_obstacle and min_ground in 1 .. 2^31 - 1."""
    w = {}
    for k in VOXEL_FLATTEN_WORDS:
        v = spec.get(k) if isinstance(spec, dict) else getattr(spec, k, None)
        w[k] = _whole(v, k + " of the flatten spec")
    reserved = spec.get("reserved", ()) if isinstance(spec, dict) else getattr(spec, "reserved", ())
    if any(int(v) != 0 for v in reserved):
        raise ValueError("a reserved word of the flatten spec is not 0: %r" % (list(reserved),))
    if w["mode"] not in (0, 1):
        raise ValueError("mode must be 0 (an absolute floor) or 1 (a local floor), got %d" % w["mode"])
    if abs(w["z_ref_q"]) >= VOXEL_FLATTEN_REF_MAX:
        raise ValueError("|z_ref_q| must stay below 2^30, got %d" % w["z_ref_q"])
    if not 1 <= w["step_q"] < w["height_q"] < VOXEL_FLATTEN_ZQ_MAX:
        raise ValueError("1 <= step_q < height_q < 2^28 must hold, got %d and %d" % (w["step_q"], w["height_q"]))
    if not 0 <= w["radius"] <= VOXEL_FLATTEN_RADIUS_MAX:
        raise ValueError("radius must lie in 0 .. 8 flat cells, got %d" % w["radius"])
    if not (1 <= w["min_obstacle"] < 2 ** 31 and 1 <= w["min_ground"] < 2 ** 31):
        raise ValueError("min_obstacle and min_ground must lie in 1 .. 2^31 - 1, got %d and %d" % (w["min_obstacle"], w["min_ground"]))
    return w


def voxel_flatten_params(voxel_params, z_ref=None, step=0.2, height=2.0, radius=2, min_obstacle=1, min_ground=1):
    """The words of a flatten (sv_voxel_flatten_spec) as a dict, from metres: voxel_params the voxel map's (its lo[2] and size), z_ref the
    height of an absolute floor in the world (mode 0; z_ref_q = floor((z_ref - lo_z) / size * 256), in zq units: 1 / 256 of a voxel cell
    above lo_z) or None for the local floor (mode 1, z_ref_q = 0: the lowest voxel within `radius` flat cells); step: what is still
    ground above and below the floor, height: from where on a voxel is overhead, both in metres, step_q and height_q = round(metres / size
    * 256); a cell is occupied from min_obstacle obstacle voxels on, else free from min_ground ground voxels on.  ValueError for a z_ref,
    step or height that is not finite and for what voxel_flatten_words refuses (step >= height, radius outside 0 .. 8, ...)."""
    lo_z, size = float(voxel_params["lo"][2]), float(voxel_params["size"])
    try:
        words = [float(step), float(height)] + ([] if z_ref is None else [float(z_ref)])
    except (TypeError, ValueError):
        raise ValueError("z_ref, step and height must be numbers, got %r, %r, %r" % (z_ref, step, height))
    if not (all(np.isfinite(v) for v in words) and np.isfinite(size) and size > 0 and np.isfinite(lo_z)):
        raise ValueError("z_ref, step and height must be finite and the voxel size > 0, got %r, %r, %r and %r" % (z_ref, step, height, size))
    q = [v / size * 256.0 for v in words]
    if any(abs(v) >= 2.0 ** 40 for v in q):
        raise ValueError("z_ref, step or height is too many voxel cells of %r m: %r, %r, %r" % (size, z_ref, step, height))
    ref_q = 0 if z_ref is None else int(np.floor((words[2] - lo_z) / size * 256.0))
    return voxel_flatten_words(dict(mode=0 if z_ref is not None else 1, z_ref_q=ref_q, step_q=int(round(q[0])), height_q=int(round(q[1])), radius=radius,
                                    min_obstacle=min_obstacle, min_ground=min_ground))


def _voxel_flatten_setup(map_state, flat_map, spec, min_n, min_rows, since):
    """What voxel_map_flatten and voxel_map_flatten_brute share: the checked words, the indices of the voxels that take part (none for an
    overflowed map) and the outputs of a map without any."""
    w, s = occupancy_map_words(flat_map), voxel_flatten_words(spec)
    if w["rows"] * w["cols"] > VOXEL_FLATTEN_CELLS_MAX:
        raise ValueError("a flat map of %d x %d cells: at most 8 000 000" % (w["rows"], w["cols"]))
    if isinstance(min_n, bool) or int(min_n) != min_n or min_n < 1:
        raise ValueError("min_n must be an integer >= 1 - a carved voxel has n = 0 and divides -, got %r" % (min_n,))
    shape = (w["rows"], w["cols"])
    out = {"logodds": np.zeros(shape, np.int16), "last_seen": np.full(shape, -1, np.int32), "floor": np.full(shape, s["z_ref_q"] if s["mode"] == 0 else -1, np.int32),
           "top": np.full(shape, -1, np.int32), "cells": np.zeros(shape + (3,), np.int32), "stats": np.zeros(8, np.int64)}
    if map_state["overflowed"]:
        out["stats"][0] = -1
        sel = np.zeros(0, np.int64)
    else:
        sel = np.flatnonzero((map_state["n"] >= min_n) & (map_state["m"] >= min_rows) & (map_state["last_seq"] >= since))
    return w, s, sel, out


def voxel_map_flatten(map_state, flat_map, spec, min_n=1, min_rows=1, since=0):
    """A voxel map sliced by height above the floor and written out in the flat map's layout, the definition of
    include/stereo_vision_hip.h (V) in numpy: what occupancy_clearance, cost_to_goal, frontier_cells and occupancy_view take.  The voxel
    map is only read.

    flat_map: occupancy_map_params' dict (or an object with its nine words), rows * cols <= 8 000 000; spec: voxel_flatten_params' dict;
    min_n >= 1, min_rows, since: voxel_map_rows' filters.  A voxel that passes them has X, Y = its centre on axes 0 and 1, lo + (c + (S +
    0.5 n) / (65536 n)) * size in double as written (voxel_map_rows' xyz), gx = floor(X ms), gy = floor(Y ms) with ms = float(scale), the
    flat cell (top - 1 - gx, left - 1 - gy) (occupancy_cells_of's rule: compared in double first; a voxel outside the flat map counts into
    `outside` and does nothing else) and the height zq = cz * 256 + ((S_z // n) >> 8), an integer < 2^28.  Behind that everything is an
    integer.  Per cell low = the least zq and seen = the largest last_seq of its voxels.  The floor: base = z_ref_q everywhere (mode 0),
    or per cell the least low over the cells within `radius` rows and columns of it that lie inside the map and hold a voxel (mode 1: a
    wall's own column has no ground voxel under it, its neighbours have).  A voxel with h = zq - base of its cell is below for h <
    -step_q (counted, and ignored in its cell; mode 0 only), ground for h < step_q, an obstacle for h < height_q and overhead from there
    on.  A cell with obstacle >= min_obstacle voxels gets L = min(l_max, obstacle * l_occ), else one with ground >= min_ground gets L =
    max(l_min, -(ground * l_free)), both with last_seen = seen; every other cell - one that holds overhead voxels only, too - L = 0 and
    last_seen = -1: unknown.

    Returns a dict: logodds int16 and last_seen int32 [rows,cols]; floor int32 [rows,cols] = base (mode 1: -1 where the window holds no
    voxel); top int32 [rows,cols] = the largest zq of the cell's ground and obstacle voxels, -1 without one; cells int32 [rows,cols,3] =
    ground, obstacle, overhead voxels; stats int64 [8] = drawn (the voxels that took part and fell inside), outside, below, ground,
    obstacle, overhead, occupied_cells, free_cells (VOXEL_FLATTEN_STATS).  An overflowed map: drawn = -1 and the outputs of a map without
    voxels."""
    w, s, sel, out = _voxel_flatten_setup(map_state, flat_map, spec, min_n, min_rows, since)
    rows, cols, R = w["rows"], w["cols"], s["radius"]
    p = map_state["params"]
    size, ms = np.float64(p["size"]), np.float64(w["scale"])
    key, n, S, last = map_state["key"][sel], map_state["n"][sel], map_state["S"][sel], map_state["last_seq"][sel]
    nf = n.astype(np.float64)
    g = []
    for k in range(2):
        c = ((key >> (20 * k)) & 0xFFFFF).astype(np.float64)
        g.append(np.floor((np.float64(p["lo"][k]) + (c + (S[:, k].astype(np.float64) + 0.5 * nf) / (65536.0 * nf)) * size) * ms))
    inside = (g[0] >= w["top"] - rows) & (g[0] <= w["top"] - 1) & (g[1] >= w["left"] - cols) & (g[1] <= w["left"] - 1)
    if not map_state["overflowed"]:
        out["stats"][:2] = int(inside.sum()), int((~inside).sum())
    cell = (w["top"] - 1 - g[0][inside].astype(np.int64)) * cols + (w["left"] - 1 - g[1][inside].astype(np.int64))
    zq = ((key[inside] >> 40) & 0xFFFFF) * 256 + ((S[inside, 2] // n[inside]) >> 8)
    low, seen = np.full(rows * cols, _VOXEL_FLATTEN_NONE, np.int64), np.full(rows * cols, -1, np.int64)
    np.minimum.at(low, cell, zq)
    np.maximum.at(seen, cell, last[inside])
    if s["mode"] == 0:
        base = np.full(rows * cols, s["z_ref_q"], np.int64)
    else:
        padded = np.full((rows + 2 * R, cols + 2 * R), _VOXEL_FLATTEN_NONE, np.int64)
        padded[R:R + rows, R:R + cols] = low.reshape(rows, cols)
        base = np.min([padded[dr:dr + rows, dc:dc + cols] for dr in range(2 * R + 1) for dc in range(2 * R + 1)], axis=0).reshape(-1)
        out["floor"][...] = np.where(base == _VOXEL_FLATTEN_NONE, -1, base).reshape(rows, cols)
    h = zq - base[cell]
    kind = np.where(h < -s["step_q"], 0, np.where(h < s["step_q"], 1, np.where(h < s["height_q"], 2, 3)))  # below, ground, obstacle, overhead
    counts = np.zeros((rows * cols, 3), np.int64)
    np.add.at(counts, (cell[kind > 0], kind[kind > 0] - 1), 1)
    top = np.full(rows * cols, -1, np.int64)
    solid = (kind == 1) | (kind == 2)
    np.maximum.at(top, cell[solid], zq[solid])
    occupied = counts[:, 1] >= s["min_obstacle"]
    free = ~occupied & (counts[:, 0] >= s["min_ground"])
    L = np.where(occupied, np.minimum(w["l_max"], counts[:, 1] * w["l_occ"]), np.where(free, np.maximum(w["l_min"], -(counts[:, 0] * w["l_free"])), 0))
    out["logodds"][...] = L.astype(np.int16).reshape(rows, cols)
    out["last_seen"][...] = np.where(occupied | free, seen, -1).astype(np.int32).reshape(rows, cols)
    out["top"][...], out["cells"][...] = top.reshape(rows, cols), counts.reshape(rows, cols, 3)
    out["stats"][2:] = [int((kind == k).sum()) for k in range(4)] + [int(occupied.sum()), int(free.sum())]
    return out


def voxel_map_flatten_brute(map_state, flat_map, spec, min_n=1, min_rows=1, since=0):
    """voxel_map_flatten's definition as plain loops over voxels and cells on Python floats and ints: the form the vectorised one is
    checked against.  Same arguments, same dict.  The local floor is spread from every cell that holds a voxel to the cells of its window
    - the window is symmetric, so that is the minimum each cell takes over its own."""
    import math
    w, s, sel, out = _voxel_flatten_setup(map_state, flat_map, spec, min_n, min_rows, since)
    rows, cols, R = w["rows"], w["cols"], s["radius"]
    p = map_state["params"]
    lo, size, ms = [float(x) for x in p["lo"]], float(p["size"]), float(w["scale"])
    voxels = {}  # (r, c) -> [(zq, last_seq), ...]
    for i in sel:
        key, n = int(map_state["key"][i]), int(map_state["n"][i])
        X, Y = (lo[k] + (float((key >> (20 * k)) & 0xFFFFF) + (float(int(map_state["S"][i, k])) + 0.5 * float(n)) / (65536.0 * float(n))) * size for k in range(2))
        gx, gy = math.floor(X * ms), math.floor(Y * ms)
        if not (w["top"] - rows <= gx <= w["top"] - 1 and w["left"] - cols <= gy <= w["left"] - 1):
            out["stats"][1] += 1
            continue
        out["stats"][0] += 1
        zq = ((key >> 40) & 0xFFFFF) * 256 + ((int(map_state["S"][i, 2]) // n) >> 8)
        voxels.setdefault((w["top"] - 1 - gx, w["left"] - 1 - gy), []).append((zq, int(map_state["last_seq"][i])))
    base = {}
    if s["mode"] == 1:
        for (r, c), held in voxels.items():
            low = min(zq for zq, _ in held)
            for rr in range(max(r - R, 0), min(r + R, rows - 1) + 1):
                for cc in range(max(c - R, 0), min(c + R, cols - 1) + 1):
                    base[rr, cc] = min(base.get((rr, cc), low), low)
        for (r, c), b in base.items():
            out["floor"][r, c] = b
    for (r, c), held in voxels.items():
        b = s["z_ref_q"] if s["mode"] == 0 else base[r, c]
        ground = obstacle = overhead = 0
        top = -1
        for zq, _ in held:
            h = zq - b
            if h < -s["step_q"]:
                out["stats"][2] += 1
                continue
            if h < s["step_q"]:
                ground += 1
            elif h < s["height_q"]:
                obstacle += 1
            else:
                overhead += 1
                continue
            top = max(top, zq)
        out["cells"][r, c], out["top"][r, c] = (ground, obstacle, overhead), top
        out["stats"][3:6] += (ground, obstacle, overhead)
        if obstacle >= s["min_obstacle"]:
            out["logodds"][r, c], out["stats"][6] = min(w["l_max"], obstacle * w["l_occ"]), out["stats"][6] + 1
        elif ground >= s["min_ground"]:
            out["logodds"][r, c], out["stats"][7] = max(w["l_min"], -(ground * w["l_free"])), out["stats"][7] + 1
        else:
            continue
        out["last_seen"][r, c] = max(seq for _, seq in held)
    return out


VOXEL_CLUSTER_WORDS = ("connectivity", "mode", "z_ref_q", "h_lo_q", "h_hi_q", "min_voxels", "capacity", "drop")  # sv_voxel_cluster_spec, in its order
VOXEL_CLUSTER_INFO = ("members", "components", "kept", "small_voxels", "emptied", "largest")  # voxel_map_clusters' info, words 0 .. 5
VOXEL_CLUSTER_ROW = ("key", "voxels", "n", "cmin_x", "cmin_y", "cmin_z", "cmax_x", "cmax_y", "cmax_z", "sum_x", "sum_y", "sum_z", "first_seq", "last_seq", "m", "zero")
VOXEL_CLUSTER_CAPACITY_MAX = 65535  # rows per call of the C entry
VOXEL_CLUSTER_BAND_MAX = 2 ** 30    # |z_ref_q|, |h_lo_q|, |h_hi_q| at most: with zq < 2^28 the height stays an int32 over an absolute floor
VOXEL_CLUSTER_SMALL, VOXEL_CLUSTER_CUT = -2, -3  # labels: a member of a component below min_voxels; of a kept component without a row
VOXEL_CLUSTER_OFFSETS = tuple((o % 3 - 1, (o // 3) % 3 - 1, o // 9 - 1) for o in range(13))  # (dx, dy, dz): the half that is negative in (dz, dy, dx) order


def voxel_cluster_words(spec):
    """The words of sv_voxel_cluster_spec as a dict of ints - VOXEL_CLUSTER_WORDS - from a dict of them (voxel_cluster_params'; a
    "reserved" entry must hold zeros only), after the checks the C entry makes (ValueError): connectivity 6, 18 or 26, mode 0 or 1,
    |z_ref_q| <= 2^30, -2^30 <= h_lo_q < h_hi_q <= 2^30, min_voxels in 1 .. 2^31 - 1, capacity in 1 .. 65535, drop 0 or 1."""
    w = {}
    for k in VOXEL_CLUSTER_WORDS:
        v = spec.get(k) if isinstance(spec, dict) else getattr(spec, k, None)
        w[k] = int(v) if k == "drop" and isinstance(v, (bool, np.bool_)) else _whole(v, k + " of the cluster spec")
    reserved = spec.get("reserved", ()) if isinstance(spec, dict) else getattr(spec, "reserved", ())
    if any(int(v) != 0 for v in reserved):
        raise ValueError("a reserved word of the cluster spec is not 0: %r" % (list(reserved),))
    if w["connectivity"] not in (6, 18, 26):
        raise ValueError("connectivity must be 6, 18 or 26, got %d" % w["connectivity"])
    if w["mode"] not in (0, 1):
        raise ValueError("mode must be 0 (an absolute floor) or 1 (the floor plane of a flatten), got %d" % w["mode"])
    if abs(w["z_ref_q"]) > VOXEL_CLUSTER_BAND_MAX:
        raise ValueError("|z_ref_q| must not exceed 2^30, got %d" % w["z_ref_q"])
    if not -VOXEL_CLUSTER_BAND_MAX <= w["h_lo_q"] < w["h_hi_q"] <= VOXEL_CLUSTER_BAND_MAX:
        raise ValueError("-2^30 <= h_lo_q < h_hi_q <= 2^30 must hold, got %d and %d" % (w["h_lo_q"], w["h_hi_q"]))
    if not 1 <= w["min_voxels"] < 2 ** 31:
        raise ValueError("min_voxels must lie in 1 .. 2^31 - 1, got %d" % w["min_voxels"])
    if not 1 <= w["capacity"] <= VOXEL_CLUSTER_CAPACITY_MAX:
        raise ValueError("capacity must lie in 1 .. 65535, got %d" % w["capacity"])
    if w["drop"] not in (0, 1):
        raise ValueError("drop must be 0 or 1, got %d" % w["drop"])
    return w


def voxel_cluster_params(voxel_params, connectivity=26, min_voxels=1, capacity=1024, mode=0, z_ref=None, h_lo=None, h_hi=None, drop=False):
    """The words of a clustering (sv_voxel_cluster_spec) as a dict, from metres: voxel_params the voxel map's (its lo[2] and size).  mode 0:
    heights count from z_ref, metres in the world (None: the box's lo[2]; z_ref_q = floor((z_ref - lo_z) / size * 256)), and h_lo, h_hi
    = None take every height (-2^30 and 2^30).  mode 1: heights count from the floor plane of a flatten, z_ref is not used, and h_lo, h_hi
    = None are the flatten's own step and height, 0.2 m and 2.0 m: its obstacle voxels.  h_lo_q and h_hi_q = round(metres / size * 256).
    ValueError for a number that is not finite and for what voxel_cluster_words refuses."""
    lo_z, size = float(voxel_params["lo"][2]), float(voxel_params["size"])
    if mode not in (0, 1):
        raise ValueError("mode must be 0 or 1, got %r" % (mode,))
    if mode == 1:
        z_ref, h_lo, h_hi = None, 0.2 if h_lo is None else h_lo, 2.0 if h_hi is None else h_hi
    try:
        given = [None if v is None else float(v) for v in (z_ref, h_lo, h_hi)]
    except (TypeError, ValueError):
        raise ValueError("z_ref, h_lo and h_hi must be numbers or None, got %r, %r, %r" % (z_ref, h_lo, h_hi))
    if not (all(v is None or np.isfinite(v) for v in given) and np.isfinite(size) and size > 0 and np.isfinite(lo_z)):
        raise ValueError("z_ref, h_lo and h_hi must be finite and the voxel size > 0, got %r, %r, %r and %r" % (z_ref, h_lo, h_hi, size))
    q = [None if v is None else v / size * 256.0 for v in given]
    if any(v is not None and abs(v) >= 2.0 ** 40 for v in q):
        raise ValueError("z_ref, h_lo or h_hi is too many voxel cells of %r m: %r, %r, %r" % (size, z_ref, h_lo, h_hi))
    return voxel_cluster_words(dict(connectivity=connectivity, mode=mode, z_ref_q=0 if given[0] is None else int(np.floor((given[0] - lo_z) / size * 256.0)),
                                    h_lo_q=-VOXEL_CLUSTER_BAND_MAX if q[1] is None else int(round(q[1])), h_hi_q=VOXEL_CLUSTER_BAND_MAX if q[2] is None else int(round(q[2])),
                                    min_voxels=min_voxels, capacity=capacity, drop=drop))


def _voxel_cluster_setup(map_state, spec, flat_map, floor, min_n, min_rows, since):
    """What voxel_map_clusters and voxel_map_clusters_brute share: the checked words, the map's entries in ascending key (`order`: indices
    into the state) and which of them are members (none for an overflowed map)."""
    s = voxel_cluster_words(spec)
    if isinstance(min_n, bool) or int(min_n) != min_n or min_n < 1:
        raise ValueError("min_n must be an integer >= 1 - an emptied voxel has n = 0 and divides -, got %r" % (min_n,))
    order = np.argsort(map_state["key"], kind="stable")
    key, n, S = map_state["key"][order], map_state["n"][order], map_state["S"][order]
    member = (n >= min_n) & (map_state["m"][order] >= min_rows) & (map_state["last_seq"][order] >= since)
    if map_state["overflowed"]:
        member[:] = False
    at = np.flatnonzero(member)
    nm = n[at]
    base = np.full(len(at), s["z_ref_q"], np.int64)
    ok = np.ones(len(at), bool)
    if s["mode"] == 1:
        if flat_map is None or floor is None:
            raise ValueError("mode 1 needs flat_map and floor: the words and the floor plane of a flatten")
        w = occupancy_map_words(flat_map)
        floor = np.asarray(floor)
        if floor.dtype != np.int32 or floor.shape != (w["rows"], w["cols"]):
            raise ValueError("floor must be int32 [%d,%d], got %s %s" % (w["rows"], w["cols"], floor.dtype, floor.shape))
        p = map_state["params"]
        size, ms, nf = np.float64(p["size"]), np.float64(w["scale"]), nm.astype(np.float64)
        g = []
        for k in range(2):
            c = ((key[at] >> (20 * k)) & 0xFFFFF).astype(np.float64)
            g.append(np.floor((np.float64(p["lo"][k]) + (c + (S[at, k].astype(np.float64) + 0.5 * nf) / (65536.0 * nf)) * size) * ms))
        ok = (g[0] >= w["top"] - w["rows"]) & (g[0] <= w["top"] - 1) & (g[1] >= w["left"] - w["cols"]) & (g[1] <= w["left"] - 1)
        r, c = np.where(ok, w["top"] - 1 - g[0], 0).astype(np.int64), np.where(ok, w["left"] - 1 - g[1], 0).astype(np.int64)
        base = floor[r, c].astype(np.int64)
        ok &= base != -1
    h = ((key[at] >> 40) & 0xFFFFF) * 256 + ((S[at, 2] // np.maximum(nm, 1)) >> 8) - base
    member[at] = ok & (s["h_lo_q"] <= h) & (h < s["h_hi_q"])
    return s, order, member


def _voxel_cluster_result(map_state, s, order, member, comp):
    """The outputs from the partition: comp int64 per member, in ascending key, = the index among the members of the component's least
    key.  Applies `drop` to the state."""
    key = map_state["key"][order]
    info, label = np.zeros(8, np.int64), np.full(len(key), -1, np.int32)
    if map_state["overflowed"]:
        info[0] = -1
        return {"clusters": np.zeros((0, 16), np.int64), "info": info, "key": key, "label": label}
    at = order[member]  # the members, into the state, in ascending key
    roots, inv, voxels = np.unique(comp, return_inverse=True, return_counts=True)  # ascending least key
    inv = inv.reshape(-1)
    keep = voxels >= s["min_voxels"]
    row = np.where(keep, np.cumsum(keep) - 1, VOXEL_CLUSTER_SMALL)
    row[keep & (row >= s["capacity"])] = VOXEL_CLUSTER_CUT
    label[member] = row[inv]
    small = ~keep[inv]
    info[:6] = [len(at), len(roots), int(keep.sum()), int(small.sum()), int(small.sum()) if s["drop"] else 0, int(voxels.max()) if len(voxels) else 0]
    R = min(int(keep.sum()), s["capacity"])
    rows = np.zeros((R, 16), np.int64)
    mine = row[inv] >= 0
    to, src = row[inv][mine], at[mine]
    k, n = map_state["key"][src], map_state["n"][src]
    cell = np.stack([(k >> (20 * a)) & 0xFFFFF for a in range(3)], -1)
    rows[:, 0], rows[:, 3:6], rows[:, 6:9], rows[:, 12], rows[:, 13] = np.iinfo(np.int64).max, np.iinfo(np.int64).max, -1, np.iinfo(np.int64).max, -1
    np.minimum.at(rows[:, 0], to, k)
    np.add.at(rows[:, 1], to, 1)
    np.add.at(rows[:, 2], to, n)
    for a in range(3):
        np.minimum.at(rows[:, 3 + a], to, cell[:, a])
        np.maximum.at(rows[:, 6 + a], to, cell[:, a])
        np.add.at(rows[:, 9 + a], to, cell[:, a] * 256 + ((map_state["S"][src, a] // n) >> 8))
    np.minimum.at(rows[:, 12], to, map_state["first_seq"][src])
    np.maximum.at(rows[:, 13], to, map_state["last_seq"][src])
    np.add.at(rows[:, 14], to, map_state["m"][src])
    if s["drop"]:
        gone = at[small]
        for f in ("n", "S", "C", "m"):
            map_state[f][gone] = 0
        map_state["first_seq"][gone], map_state["last_seq"][gone] = np.iinfo(np.int64).max, -1
    return {"clusters": rows, "info": info, "key": key, "label": label}


def voxel_map_clusters(map_state, spec, flat_map=None, floor=None, min_n=1, min_rows=1, since=0):
    """The connected components of a voxel map, the definition of include/stereo_vision_hip.h (W) in numpy; integers throughout but for
    the flat cell of mode 1.  map_state (voxel_map_state's dict) is changed under spec["drop"] only.

    spec: voxel_cluster_params' dict.  A voxel is a member iff n >= min_n (>= 1: an emptied voxel never is), m >= min_rows, last_seq >=
    since and h_lo_q <= zq - base < h_hi_q with zq = cz * 256 + ((S_z // n) >> 8), voxel_map_flatten's, and base = z_ref_q (mode 0) or
    floor[cell] (mode 1): floor the int32 [rows,cols] floor plane of voxel_map_flatten on flat_map, cell the flat cell under the voxel's
    centre by voxel_map_flatten's rule; a voxel outside flat_map or over a cell with floor -1 is no member.  Two members are neighbours
    iff their cells differ by at most 1 on every axis, on 1 (connectivity 6), up to 2 (18) or up to 3 (26) axes; the cells are tested
    against the box per axis before a key is made of them.  A component is the transitive closure; its identity is its least key.

    Sorted keys, searchsorted neighbours over VOXEL_CLUSTER_OFFSETS, least-label propagation with pointer jumping to a fixed point.

    Returns a dict: clusters int64 [R,16], R = min(kept, capacity): the components with voxels >= min_voxels in ascending least key, cut
    to `capacity` - the cut is made behind the order, so the rows are the least keys - with the words VOXEL_CLUSTER_ROW (least key,
    voxels, sum n, least and largest cell per axis, sum over the members of c_k * 256 + ((S_k // n) >> 8) per axis, least first_seq,
    largest last_seq, sum m, 0); info int64 [8] = members, components, kept, voxels in components below min_voxels, voxels emptied,
    voxels of the largest component, 0, 0; key int64 [V], every entry of the map in ascending key, and label int32 [V], its row, -1 for
    no member, -2 in a component below min_voxels, -3 in a kept component behind the cut.  drop: the members labelled -2 are emptied as
    voxel_map_carve empties.  An overflowed map: info[0] = -1, no rows, every label -1, nothing done."""
    s, order, member = _voxel_cluster_setup(map_state, spec, flat_map, floor, min_n, min_rows, since)
    cells = np.array(map_state["params"]["cells"], np.int64)
    mk = map_state["key"][order][member]
    M = len(mk)
    c = np.stack([(mk >> (20 * a)) & 0xFFFFF for a in range(3)], -1) if M else np.zeros((0, 3), np.int64)
    most = {6: 1, 18: 2, 26: 3}[s["connectivity"]]
    ei, ej = [], []
    for d in VOXEL_CLUSTER_OFFSETS:
        if sum(v != 0 for v in d) > most or not M:
            continue
        nb = c + np.array(d, np.int64)
        inside = ((nb >= 0) & (nb < cells)).all(-1)  # per axis, before a key is made
        nkey = nb[:, 0] | (nb[:, 1] << 20) | (nb[:, 2] << 40)
        at = np.minimum(np.searchsorted(mk, nkey), M - 1)
        hit = inside & (mk[at] == nkey)
        ei.append(np.flatnonzero(hit)), ej.append(at[hit])
    ei, ej = (np.concatenate(ei), np.concatenate(ej)) if ei else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    lab = np.arange(M, dtype=np.int64)
    while True:
        new = lab.copy()
        np.minimum.at(new, ei, lab[ej])
        np.minimum.at(new, ej, lab[ei])
        while True:  # pointer jumping
            jumped = new[new]
            if (jumped == new).all():
                break
            new = jumped
        if (new == lab).all():
            break
        lab = new
    return _voxel_cluster_result(map_state, s, order, member, lab)


def voxel_map_clusters_brute(map_state, spec, flat_map=None, floor=None, min_n=1, min_rows=1, since=0):
    """voxel_map_clusters' definition as a plain flood fill over a dict of cells: the form the vectorised one is checked against.  Same
    arguments, same dict."""
    s, order, member = _voxel_cluster_setup(map_state, spec, flat_map, floor, min_n, min_rows, since)
    cells = [int(v) for v in map_state["params"]["cells"]]
    mk = [int(k) for k in map_state["key"][order][member]]
    where = {(k & 0xFFFFF, (k >> 20) & 0xFFFFF, (k >> 40) & 0xFFFFF): i for i, k in enumerate(mk)}
    most = {6: 1, 18: 2, 26: 3}[s["connectivity"]]
    steps = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if 1 <= (dx != 0) + (dy != 0) + (dz != 0) <= most]
    comp = [-1] * len(mk)
    for cell, i in sorted(where.items(), key=lambda item: item[1]):  # ascending key: a fill starts at its component's least
        if comp[i] >= 0:
            continue
        comp[i], stack = i, [cell]
        while stack:
            x, y, z = stack.pop()
            for dx, dy, dz in steps:
                nb = (x + dx, y + dy, z + dz)
                if not all(0 <= nb[a] < cells[a] for a in range(3)):
                    continue
                j = where.get(nb)
                if j is not None and comp[j] < 0:
                    comp[j] = i
                    stack.append(nb)
    return _voxel_cluster_result(map_state, s, order, member, np.array(comp, np.int64).reshape(-1))


def voxel_cluster_boxes(clusters, params):
    """Cluster rows in metres, in double on the host: clusters int64 [R,16] (voxel_map_clusters' rows), params the voxel map's.  -> a dict
    of float64 [R,3] arrays: centre = lo + (sum_q / voxels) / 256 * size, the mean of the members' mean positions; lo and hi = the box's
    corners, lo + cmin * size and lo + (cmax + 1) * size - and of int64 [R] arrays key, voxels, n, first_seq, last_seq."""
    rows = np.asarray(clusters, np.int64).reshape(-1, 16)
    lo, size = np.array(params["lo"], np.float64), np.float64(params["size"])
    voxels = rows[:, 1].astype(np.float64)[:, None]
    return {"centre": lo + (rows[:, 9:12].astype(np.float64) / voxels) / 256.0 * size, "lo": lo + rows[:, 3:6].astype(np.float64) * size,
            "hi": lo + (rows[:, 6:9].astype(np.float64) + 1.0) * size, "key": rows[:, 0].copy(), "voxels": rows[:, 1].copy(), "n": rows[:, 2].copy(),
            "first_seq": rows[:, 12].copy(), "last_seq": rows[:, 13].copy()}


VOXEL_MATCH_BATCH_MAX = 65535
VOXEL_MATCH_POSES_MAX = 65535  # candidates per frame of voxel_map_match
_VOXEL_MATCH_BLOCK = 1 << 18   # row x candidate pairs voxel_map_match holds at a time


def voxel_map_pose_window(x, y, z, yaw, half, steps):
    """float64 [P, 4] = (x, y, z, yaw): the candidates of a window around the guess (x, y, z, yaw) - occupancy_pose_window's rule on four
    axes: half = (dx, dy, dz, dyaw), the window's half widths (metres, metres, metres, radians; finite, >= 0), steps = (nx, ny, nz, nyaw),
    odd integers >= 1 with P = nx ny nz nyaw <= 65535.  Row 0 is the guess itself, so that ties keep it; the other P - 1 follow in
    row-major (i, j, k, l) order over numpy.linspace(-half, +half, n) per axis (n = 1: the offset 0), the middle one - the guess - left
    out.  voxel_map_pose(x, y, yaw, z) turns the rows into poses."""
    g = [float(v) for v in (x, y, z, yaw)]
    if len(half) != 4 or len(steps) != 4:
        raise ValueError("half and steps must have four entries each, got %r, %r" % (half, steps))
    h = [float(v) for v in half]
    if not all(np.isfinite(v) for v in g + h) or min(h) < 0:
        raise ValueError("the guess and half must be finite and half >= 0, got %r, %r" % (g, h))
    for v in steps:
        if isinstance(v, (bool, np.bool_)) or int(v) != v or v < 1 or int(v) % 2 != 1:
            raise ValueError("steps must be odd integers >= 1, got %r" % (steps,))
    n = [int(v) for v in steps]
    if n[0] * n[1] * n[2] * n[3] > VOXEL_MATCH_POSES_MAX:
        raise ValueError("a window of %d poses: at most 65535" % (n[0] * n[1] * n[2] * n[3]))
    off = [np.linspace(-h[a], h[a], n[a]) if n[a] > 1 else np.zeros(1) for a in range(4)]
    grid = np.stack(np.meshgrid(*[g[a] + off[a] for a in range(4)], indexing="ij"), -1).reshape(-1, 4)
    mid = ((n[0] // 2 * n[1] + n[1] // 2) * n[2] + n[2] // 2) * n[3] + n[3] // 2
    return np.concatenate([np.array([g]), grid[:mid], grid[mid + 1:]])


def voxel_map_match(map_state, xyz, n, counts, poses, min_n=1, min_rows=1, since=0):
    """The definition of include/stereo_vision_hip.h (R) in numpy: the rows of B frames scored against a voxel map at P candidate poses
    per frame.  map_state, xyz (float32 or float64 [B,cap,3]), n (int32 [B,cap], or None: every weight 1) and counts (int32 [B]) are
    voxel_map_insert's; poses float64 [B,P,12] in voxel_map_pose's layout ([P,12] accepted for one frame), 1 <= P <= 65535, B <= 65535,
    B P < 2^31 (ValueError).  The map is not changed.
    -> {"inside": int32 [B,P], "hits": int32 [B,P], "weight": int64 [B,P], "d2": int64 [B,P], "best": int32 [B], "best_weight": int64 [B],
        "best_d2": int64 [B]}.

      rows    frame b has its first min(counts[b], cap) rows, none for counts[b] <= 0; a row's weight w is n[b][i], or 1.
      world   Pw[k] = ((R[k,0] x + R[k,1] y) + R[k,2] z) + t[k] under candidate p, in double and in that order: voxel_map_insert's.
      kept    w > 0 and lo < Pw < hi strictly on every axis (NaN, inf and a pose with a word that is not finite keep nothing); inside
              counts the kept rows.
      cell    the insert's: t = (Pw - lo) / size, c = min(int(t), cells - 1), u = min(int((t - c) * 65536), 65535), key = cx | cy << 20
              | cz << 40.
      hit     the map holds a voxel of that key with n >= min_n, m >= min_rows and last_seq >= since - voxel_map_rows' filters; hits
              counts the kept rows that hit, weight adds up their w, and d2 adds up, unweighted, (u_k - S_k // n)^2 over the three axes
              with the voxel's S and n: the squared distance, in 1 / 65536 of a cell, to the floor of the voxel's mean offset.
      best    the candidate with the largest weight, among those the smallest d2, among those the lowest p.
    For an overflowed map every per-candidate output is 0, best -1, best_weight and best_d2 0."""
    w = map_state["params"]
    lo, hi, size, cells = np.array(w["lo"]), np.array(w["hi"]), np.float64(w["size"]), np.array(w["cells"], np.int64)
    xyz = np.asarray(xyz)
    if xyz.dtype not in (np.float32, np.float64) or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be float32 or float64 [B,cap,3], got %s %s" % (xyz.dtype, xyz.shape))
    B, cap = xyz.shape[:2]
    counts = np.asarray(counts)
    if counts.shape != (B,):
        raise ValueError("counts must be [%d], got %s" % (B, counts.shape))
    if n is not None and np.asarray(n).shape != (B, cap):
        raise ValueError("n must be [B,cap] or None")
    p = np.asarray(poses, np.float64)
    if p.ndim == 2 and B == 1:
        p = p[None]
    if p.ndim != 3 or p.shape[0] != B or p.shape[2] != 12:
        raise ValueError("poses must be float64 [%d, P, 12], got %s" % (B, p.shape))
    P = p.shape[1]
    if B > VOXEL_MATCH_BATCH_MAX or not 1 <= P <= VOXEL_MATCH_POSES_MAX or B * P >= 2 ** 31:
        raise ValueError("at most 65535 frames of 1 .. 65535 poses each and fewer than 2^31 in all, got %d x %d" % (B, P))
    out = {"inside": np.zeros((B, P), np.int32), "hits": np.zeros((B, P), np.int32), "weight": np.zeros((B, P), np.int64), "d2": np.zeros((B, P), np.int64)}
    if map_state["overflowed"]:
        return dict(out, best=np.full(B, -1, np.int32), best_weight=np.zeros(B, np.int64), best_d2=np.zeros(B, np.int64))
    sel = (map_state["n"] >= min_n) & (map_state["m"] >= min_rows) & (map_state["last_seq"] >= since)
    by_key = np.argsort(map_state["key"][sel], kind="stable")
    vkey = map_state["key"][sel][by_key]
    vmean = (map_state["S"][sel] // map_state["n"][sel][:, None])[by_key]
    for b in range(B):
        rows = int(min(max(int(counts[b]), 0), cap))
        if rows == 0:
            continue
        X = xyz[b, :rows].astype(np.float64)
        x, y, z = X[None, :, 0], X[None, :, 1], X[None, :, 2]
        wt = np.ones(rows, np.int64) if n is None else np.asarray(n)[b, :rows].astype(np.int64)
        step = max(1, _VOXEL_MATCH_BLOCK // rows)
        for p0 in range(0, P, step):
            R = p[b, p0:p0 + step, None, :]
            with np.errstate(invalid="ignore", over="ignore"):
                Pw = np.stack([((R[..., 3 * k] * x + R[..., 3 * k + 1] * y) + R[..., 3 * k + 2] * z) + R[..., 9 + k] for k in range(3)], -1)
                keep = ((lo < Pw) & (Pw < hi)).all(-1) & (wt > 0)[None, :]  # [candidates, rows]
            t = (Pw[keep] - lo) / size
            c = np.minimum(t.astype(np.int64), cells - 1)
            u = np.minimum(((t - c.astype(np.float64)) * 65536.0).astype(np.int64), 65535)
            key = c[:, 0] | (c[:, 1] << 20) | (c[:, 2] << 40)
            at = np.minimum(np.searchsorted(vkey, key), max(len(vkey) - 1, 0))
            hit = vkey[at] == key if len(vkey) else np.zeros(len(key), bool)
            cand, row = np.nonzero(keep)
            d = u[hit] - vmean[at[hit]] if len(vkey) else np.zeros((0, 3), np.int64)
            m = R.shape[0]
            out["inside"][b, p0:p0 + m] = keep.sum(1)
            out["hits"][b, p0:p0 + m] = np.bincount(cand[hit], minlength=m)
            np.add.at(out["weight"][b, p0:p0 + m], cand[hit], wt[row[hit]])
            np.add.at(out["d2"][b, p0:p0 + m], cand[hit], (d * d).sum(1))
    order = [np.lexsort((np.arange(P), out["d2"][b], -out["weight"][b]))[0] for b in range(B)]
    best = np.array(order, np.int64)
    at = np.arange(B)
    return dict(out, best=best.astype(np.int32), best_weight=out["weight"][at, best] if B else np.zeros(0, np.int64),
                best_d2=out["d2"][at, best] if B else np.zeros(0, np.int64))


VOXEL_ALIGN_BATCH_MAX = 65535
VOXEL_ALIGN_D2_MAX = 3 * 511 ** 2  # 783363: the largest d2 between a row and a voxel of its 27 cells
VOXEL_ALIGN_ORIGIN_MAX = 2 ** 30   # |origin| per axis at most: p - o and q - o stay 32-bit numbers
VOXEL_ALIGN_SUMS = ("inside", "pairs", "W", "D", "Px", "Py", "Pz", "Qx", "Qy", "Qz", "Hxx", "Hxy", "Hxz", "Hyx", "Hyy", "Hyz", "Hzx", "Hzy", "Hzz")  # the 19 words
VOXEL_ALIGN_OFFSETS = tuple((o % 3 - 1, (o // 3) % 3 - 1, o // 9 - 1) for o in range(27))  # (dx, dy, dz) of the 27 cells


def voxel_align_max_d2(max_dist):
    """max_d2 = min(783363, int((256 max_dist)^2)) of a max_dist in cells: finite and >= 0 (ValueError)."""
    try:
        m = float(max_dist)
    except (TypeError, ValueError):
        raise ValueError("max_dist must be a finite number of cells >= 0, got %r" % (max_dist,))
    if not np.isfinite(m) or m < 0:
        raise ValueError("max_dist must be a finite number of cells >= 0, got %r" % (max_dist,))
    return min(VOXEL_ALIGN_D2_MAX, int((256.0 * min(m, 4.0)) ** 2))


def _voxel_align_setup(map_state, xyz, n, counts, poses, origin):
    """The checks voxel_map_align_sums and its brute form share -> (xyz, n, counts, poses [B,12], origin int64 [B,3])."""
    xyz = np.asarray(xyz)
    if xyz.dtype not in (np.float32, np.float64) or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be float32 or float64 [B,cap,3], got %s %s" % (xyz.dtype, xyz.shape))
    B, cap = xyz.shape[:2]
    if B > VOXEL_ALIGN_BATCH_MAX:
        raise ValueError("at most 65535 frames per call, got %d" % B)
    counts = np.asarray(counts)
    if counts.shape != (B,):
        raise ValueError("counts must be [%d], got %s" % (B, counts.shape))
    if n is not None and np.asarray(n).shape != (B, cap):
        raise ValueError("n must be [B,cap] or None")
    p = np.asarray(poses, np.float64)
    if p.ndim != 2 or p.shape[0] != B or p.shape[1] not in (4, 12):
        raise ValueError("poses must be float64 [%d,12] or [%d,4], got %s" % (B, B, p.shape))
    p = voxel_map_pose_words(p) if B else np.zeros((0, 12))
    o = np.asarray(origin)
    if o.shape != (B, 3) or o.dtype.kind not in "iu" or (np.abs(o.astype(np.int64)) > VOXEL_ALIGN_ORIGIN_MAX).any():
        raise ValueError("origin must be integers [%d,3] within +-2^30, got %s %s" % (B, o.dtype, o.shape))
    return xyz, None if n is None else np.asarray(n), counts, p, o.astype(np.int64)


def _voxel_align_voxels(map_state, min_n, min_rows, since):
    """(key, q) of the voxels a row may pair with, in ascending key: q int64 [V,3] = 256 cell + ((S // n) >> 8)."""
    sel = (map_state["n"] >= max(min_n, 1)) & (map_state["m"] >= min_rows) & (map_state["last_seq"] >= since)
    key, n, S = map_state["key"][sel], map_state["n"][sel], map_state["S"][sel]
    by_key = np.argsort(key, kind="stable")
    key, n, S = key[by_key], n[by_key], S[by_key]
    cell = np.stack([key & 0xFFFFF, (key >> 20) & 0xFFFFF, (key >> 40) & 0xFFFFF], -1)
    return key, 256 * cell + ((S // n[:, None]) >> 8)


def _voxel_align_rows(params, X, wt, pose):
    """The kept rows of one frame under `pose` -> (their indices, c int64 [K,3], p int64 [K,3]): voxel_map_match's rules."""
    lo, hi, size, cells = np.array(params["lo"]), np.array(params["hi"]), np.float64(params["size"]), np.array(params["cells"], np.int64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        Pw = np.stack([((pose[3 * k] * x + pose[3 * k + 1] * y) + pose[3 * k + 2] * z) + pose[9 + k] for k in range(3)], -1)
        keep = ((lo < Pw) & (Pw < hi)).all(-1) & (wt > 0)
    t = (Pw[keep] - lo) / size
    c = np.minimum(t.astype(np.int64), cells - 1)
    u = np.minimum(((t - c.astype(np.float64)) * 65536.0).astype(np.int64), 65535)
    return np.flatnonzero(keep), c, 256 * c + (u >> 8)


def _voxel_align_nearest(cells, vkey, vq, c, p):
    """The nearest candidate of every kept row -> (d2, key, q): the voxels (vkey ascending, vq) of the up to 27 cells around the row's cell
    c, the smallest d2 to the row's position p, then the smallest key; key -1 for a row without a candidate."""
    K = len(c)
    best_d2, best_key, best_q = np.full(K, VOXEL_ALIGN_D2_MAX + 1, np.int64), np.full(K, -1, np.int64), np.zeros((K, 3), np.int64)
    for d in VOXEL_ALIGN_OFFSETS:
        cc = c + np.array(d, np.int64)
        on = ((cc >= 0) & (cc < cells)).all(-1)  # before a key is formed: a cell of -1 or of `cells` is no cell
        key = np.where(on, cc[:, 0] | (cc[:, 1] << 20) | (cc[:, 2] << 40), -2)
        at = np.minimum(np.searchsorted(vkey, key), len(vkey) - 1)
        q = vq[at]
        d2 = ((p - q) ** 2).sum(1)
        take = on & (vkey[at] == key) & ((best_key < 0) | (d2 < best_d2) | ((d2 == best_d2) & (key < best_key)))
        best_d2[take], best_key[take], best_q[take] = d2[take], key[take], q[take]
    return best_d2, best_key, best_q


def _voxel_align_add(sums, wt, p, q, d2, o):
    """The pairs of one frame added up: 64-bit two's complement sums."""
    with np.errstate(over="ignore"):
        dp, dq = p - o, q - o
        sums[1], sums[2], sums[3] = len(wt), wt.sum(), (wt * d2).sum()
        sums[4:7], sums[7:10] = (wt[:, None] * dp).sum(0), (wt[:, None] * dq).sum(0)
        sums[10:19] = ((wt[:, None] * dp)[:, :, None] * dq[:, None, :]).sum(0).reshape(9)


def voxel_map_align_sums(map_state, xyz, n, counts, poses, origin, max_dist=1.0, min_n=1, min_rows=1, since=0):
    """The definition of include/stereo_vision_hip.h (X) in numpy: the rows of B frames, each under its one pose, paired with the nearest
    voxels of a voxel map, and the pairs' sums - what one round of iterative closest point needs.  map_state, xyz (float32 or float64
    [B,cap,3]), n (int32 [B,cap], or None: every weight 1) and counts (int32 [B]) are voxel_map_insert's; poses float64 [B,12] in
    voxel_map_pose's layout ([B,4] goes through voxel_map_pose_words); origin integers [B,3] in 1/256 of a cell from lo, |o| <= 2^30
    (voxel_align_origin); B <= 65535 (ValueError).  The map is not changed.
    -> {"sums": int64 [B,19], "pair_key": int64 [B,cap], "pair_d2": int32 [B,cap]}.

      rows, world, kept, cell, offset   exactly voxel_map_match's: the insert's transform in double and in that order, strict lo < Pw <
              hi, w > 0, c = min(int(t), cells - 1), u = min(int((t - c) * 65536), 65535).  sums[b][0] = inside counts the kept rows.
      positions  integers from here on, in 1/256 of a cell from lo and below 2^28: a kept row stands at p_k = 256 c_k + (u_k >> 8), a
              voxel at q_k = 256 cell_k + ((S_k // n) >> 8) - what voxel_map_flatten slices by.
      candidates the voxels of the up to 27 cells c + d, d in {-1, 0, 1}^3, 0 <= c_k + d_k < cells_k, that pass voxel_map_rows' filters
              with n >= max(min_n, 1): a tombstone that voxel_map_carve or a despeckle left has n = 0 and is never a partner.
      nearest the candidate with the smallest d2 = sum_k (p_k - q_k)^2, then the smallest key; d2 <= 3 * 511^2 = 783363.
      pair    a kept row with a nearest candidate and d2 <= max_d2 = min(783363, int((256 max_dist)^2)); max_dist in cells, finite and
              >= 0 (ValueError).  For max_dist <= 1 the partner is the nearest voxel mean of the whole map, not only of the 27 cells: a
              voxel within 256 units differs by at most one cell per axis.
      sums    inside, pairs, W = sum w, D = sum w d2, P[3] = sum w (p - o), Q[3] = sum w (q - o), H[9] = sum w (p - o)_i (q - o)_j
              row-major, over the pairs; 64-bit two's complement sums.  Contract: sum w r^2 < 2^63, r the largest |p - o| or |q - o|.
      per row pair_key, pair_d2: the nearest candidate's key and d2, also where d2 > max_d2 and the row is no pair; -1 and -1 for a row
              that is not kept, a kept row with no candidate, and every index at or beyond min(counts[b], cap).
    For an overflowed map every sum is 0 and every per-row word is -1."""
    max_d2 = voxel_align_max_d2(max_dist)
    xyz, n, counts, poses, origin = _voxel_align_setup(map_state, xyz, n, counts, poses, origin)
    B, cap = xyz.shape[:2]
    out = {"sums": np.zeros((B, 19), np.int64), "pair_key": np.full((B, cap), -1, np.int64), "pair_d2": np.full((B, cap), -1, np.int32)}
    if map_state["overflowed"]:
        return out
    w = map_state["params"]
    cells = np.array(w["cells"], np.int64)
    vkey, vq = _voxel_align_voxels(map_state, min_n, min_rows, since)
    if not len(vkey):  # a stand-in that no cell's key equals
        vkey, vq = np.array([-1], np.int64), np.zeros((1, 3), np.int64)
    for b in range(B):
        rows = int(min(max(int(counts[b]), 0), cap))
        wt = np.ones(rows, np.int64) if n is None else n[b, :rows].astype(np.int64)
        at_row, c, p = _voxel_align_rows(w, xyz[b, :rows].astype(np.float64), wt, poses[b])
        out["sums"][b, 0] = len(at_row)
        best_d2, best_key, best_q = _voxel_align_nearest(cells, vkey, vq, c, p)
        have = best_key >= 0
        out["pair_key"][b, at_row[have]] = best_key[have]
        out["pair_d2"][b, at_row[have]] = best_d2[have]
        pair = have & (best_d2 <= max_d2)
        _voxel_align_add(out["sums"][b], wt[at_row[pair]], p[pair], best_q[pair], best_d2[pair], origin[b])
    return out


def voxel_map_align_sums_brute(map_state, xyz, n, counts, poses, origin, max_dist=1.0, min_n=1, min_rows=1, since=0):
    """voxel_map_align_sums by a Python loop per row over all voxels of the map that differ from the row's cell by at most one cell per
    axis: Python floats and ints only, no key is formed for a neighbour cell and nothing is looked up.  The independent model."""
    max_d2 = voxel_align_max_d2(max_dist)
    xyz, n, counts, poses, origin = _voxel_align_setup(map_state, xyz, n, counts, poses, origin)
    B, cap = xyz.shape[:2]
    out = {"sums": np.zeros((B, 19), np.int64), "pair_key": np.full((B, cap), -1, np.int64), "pair_d2": np.full((B, cap), -1, np.int32)}
    if map_state["overflowed"]:
        return out
    w = map_state["params"]
    voxels = []
    for key, vn, S, m, last in zip(map_state["key"].tolist(), map_state["n"].tolist(), map_state["S"].tolist(), map_state["m"].tolist(), map_state["last_seq"].tolist()):
        if vn >= max(min_n, 1) and m >= min_rows and last >= since:
            cell = [(key >> (20 * k)) & 0xFFFFF for k in range(3)]
            voxels.append((key, cell, [256 * cell[k] + ((S[k] // vn) >> 8) for k in range(3)]))
    wrap = lambda v: (v + 2 ** 63) % 2 ** 64 - 2 ** 63  # noqa: E731
    for b in range(B):
        pose, o = [float(v) for v in poses[b]], [int(v) for v in origin[b]]
        sums = [0] * 19
        for i in range(max(0, min(int(counts[b]), cap))):
            wt = 1 if n is None else int(n[b, i])
            if wt <= 0:
                continue
            x, y, z = (float(v) for v in xyz[b, i])
            c, p = [], []
            for k in range(3):
                with np.errstate(all="ignore"):
                    Pw = float(((np.float64(pose[3 * k]) * x + np.float64(pose[3 * k + 1]) * y) + np.float64(pose[3 * k + 2]) * z) + np.float64(pose[9 + k]))
                if not (w["lo"][k] < Pw < w["hi"][k]):
                    break
                t = (Pw - w["lo"][k]) / w["size"]
                c.append(min(int(t), w["cells"][k] - 1))
                p.append(256 * c[k] + (min(int((t - float(c[k])) * 65536.0), 65535) >> 8))
            if len(c) < 3:
                continue
            sums[0] += 1
            best = None
            for key, cell, q in voxels:
                if all(abs(cell[k] - c[k]) <= 1 for k in range(3)):
                    d2 = sum((p[k] - q[k]) ** 2 for k in range(3))
                    if best is None or (d2, key) < best[:2]:
                        best = (d2, key, q)
            if best is None:
                continue
            out["pair_key"][b, i], out["pair_d2"][b, i] = best[1], best[0]
            if best[0] <= max_d2:
                dp, dq = [p[k] - o[k] for k in range(3)], [best[2][k] - o[k] for k in range(3)]
                sums[1] += 1
                sums[2] += wt
                sums[3] += wt * best[0]
                for k in range(3):
                    sums[4 + k] += wt * dp[k]
                    sums[7 + k] += wt * dq[k]
                    for j in range(3):
                        sums[10 + 3 * k + j] += wt * dp[k] * dq[j]
        out["sums"][b] = [wrap(v) for v in sums]
    return out


def voxel_align_origin(params, poses):
    """int32 [B,3]: the origin the sums of voxel_map_align_sums are taken about - floor((t - lo) / size * 256) of each pose's translation,
    in 1/256 of a cell from lo, clamped into +-2^30 (0 for a word that is not finite).  An origin at the sensor keeps the sums small."""
    p = voxel_map_pose_words(poses) if len(np.asarray(poses)) else np.zeros((0, 12))
    with np.errstate(invalid="ignore", over="ignore"):
        o = np.floor((p[:, 9:] - np.array(params["lo"])) / np.float64(params["size"]) * 256.0)
    o = np.where(np.isfinite(o), o, 0.0)
    return np.clip(o, -VOXEL_ALIGN_ORIGIN_MAX, VOXEL_ALIGN_ORIGIN_MAX).astype(np.int32)


def voxel_align_solve(sums, poses, origin, params, dof=6, min_pairs=6):
    """The closed-form rigid fit of one round: from the sums of voxel_map_align_sums, the poses they were taken under and their origin
    -> (poses' float64 [B,12], ok bool [B], step float64 [B,2]).  The centred cross-covariance W H_ij - P_i Q_j is formed exactly in
    Python integers and then divided by W in double.  dof=6: Kabsch - the SVD U S V^T of the centred H, R_d = V diag(1, 1, det(V U^T))
    U^T; dof=4: the rotation about z alone, by atan2(H01 - H10, H00 + H11).  t_d = Q / W - R_d P / W, and the new pose is (R_d R, R_d (t -
    X_o) + X_o + t_d size / 256) with X_o = lo + o size / 256.  step = (the angle of R_d in radians, |t_d| in cells).  A frame with pairs
    < min_pairs, or whose sums give no finite fit, keeps its pose: ok False and step 0 for it."""
    if dof not in (4, 6) or isinstance(dof, bool):
        raise ValueError("dof must be 6 (all of the rotation) or 4 (yaw only), got %r" % (dof,))
    if isinstance(min_pairs, bool) or int(min_pairs) != min_pairs:
        raise ValueError("min_pairs must be an integer, got %r" % (min_pairs,))
    sums, poses = np.asarray(sums), voxel_map_pose_words(poses) if len(np.asarray(poses)) else np.zeros((0, 12))
    B = len(poses)
    origin = np.asarray(origin)
    if sums.shape != (B, 19) or origin.shape != (B, 3):
        raise ValueError("sums must be [%d,19] and origin [%d,3], got %s and %s" % (B, B, sums.shape, origin.shape))
    lo, size = np.array(params["lo"]), np.float64(params["size"])
    out, ok, step = poses.copy(), np.zeros(B, bool), np.zeros((B, 2))
    for b in range(B):
        s = [int(v) for v in sums[b]]
        W = s[2]
        if s[1] < max(int(min_pairs), 1) or W <= 0:
            continue
        P, Q = s[4:7], s[7:10]
        H = np.array([[(W * s[10 + 3 * i + j] - P[i] * Q[j]) / W for j in range(3)] for i in range(3)])  # exact numerators, one rounding each
        if dof == 6:
            try:
                U, _, Vt = np.linalg.svd(H)
            except np.linalg.LinAlgError:
                continue
            V = Vt.T
            Rd = V @ np.diag([1.0, 1.0, 1.0 if np.linalg.det(V @ U.T) > 0 else -1.0]) @ U.T
            axis = np.array([Rd[2, 1] - Rd[1, 2], Rd[0, 2] - Rd[2, 0], Rd[1, 0] - Rd[0, 1]])
            angle = float(np.arctan2(0.5 * np.sqrt((axis * axis).sum()), 0.5 * (np.trace(Rd) - 1.0)))
        else:
            theta = float(np.arctan2(H[0, 1] - H[1, 0], H[0, 0] + H[1, 1]))
            c, sn = np.cos(theta), np.sin(theta)
            Rd, angle = np.array([[c, -sn, 0.0], [sn, c, 0.0], [0.0, 0.0, 1.0]]), abs(theta)
        td = np.array([Q[k] / W for k in range(3)]) - Rd @ np.array([P[k] / W for k in range(3)])
        Xo = lo + origin[b].astype(np.float64) * size / 256.0
        new = np.concatenate([(Rd @ poses[b, :9].reshape(3, 3)).reshape(9), Rd @ (poses[b, 9:] - Xo) + Xo + td * size / 256.0])
        if not np.isfinite(new).all():
            continue
        out[b], ok[b], step[b] = new, True, (angle, float(np.sqrt((td * td).sum())) / 256.0)
    return out, ok, step


def voxel_align_loop(sums_of, params, poses, iterations=10, dof=6, min_pairs=6, eps=(1e-5, 1.0 / 256), solver=None):
    """The loop of voxel_map_align around any source of sums - sums_of(poses [B,12], origin [B,3]) -> int64 [B,19]: the numpy definition's
    or the device's, read back.  Everything else is host numpy, the same for both.  solver: None for the point-to-point fit of
    voxel_align_solve on 19 words, or a dict as VOXEL_ALIGN_PLANE - the words per frame, the fit, which words hold the pairs that count,
    W and the sum of squares, and the length of one unit of that square root in 1/256 of a cell."""
    solver = VOXEL_ALIGN_POINT if solver is None else solver
    words, solve, at_pairs, at_W, at_D, unit = (solver[k] for k in ("words", "solve", "pairs", "W", "D", "unit"))
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 0:
        raise ValueError("iterations must be an integer >= 0, got %r" % (iterations,))
    if dof not in (4, 6) or isinstance(dof, bool):
        raise ValueError("dof must be 6 (all of the rotation) or 4 (yaw only), got %r" % (dof,))
    if len(eps) != 2 or not all(np.isfinite(float(e)) and float(e) >= 0 for e in eps):
        raise ValueError("eps must be two finite numbers >= 0: radians and cells, got %r" % (eps,))
    poses = voxel_map_pose_words(poses) if len(np.asarray(poses)) else np.zeros((0, 12))
    B = len(poses)
    sums, ok = np.zeros((B, words), np.int64), np.zeros(B, bool)
    pairs, rms, rounds = [], [], 0
    size = np.float64(params["size"])
    for _ in range(int(iterations)):
        origin = voxel_align_origin(params, poses)
        sums = np.ascontiguousarray(sums_of(poses, origin), np.int64)
        poses, ok, step = solve(sums, poses, origin, params, dof, min_pairs)
        rounds += 1
        W, D = sums[:, at_W].astype(np.float64), sums[:, at_D].astype(np.float64)
        pairs.append(sums[:, at_pairs].copy())
        rms.append(np.where(W > 0, np.sqrt(D / np.maximum(W, 1.0)) * unit * size / 256.0, 0.0))
        if ((step[ok, 0] < eps[0]) & (step[ok, 1] < eps[1])).all():
            break
    return {"poses": poses, "ok": ok, "sums": sums, "rounds": rounds, "pairs": np.array(pairs, np.int64).reshape(rounds, B), "rms": np.array(rms, np.float64).reshape(rounds, B)}


VOXEL_ALIGN_POINT = dict(words=19, solve=voxel_align_solve, pairs=1, W=2, D=3, unit=1.0)  # voxel_align_loop's solver=None
VOXEL_ALIGN_METHODS = ("point", "plane")
VOXEL_ALIGN_PLANE_EPS = (1e-4, 1.0 / 256)  # the plane step settles near 2e-5 rad: the pairs flicker by quantisation


def voxel_map_align(map_state, xyz, n, counts, poses, iterations=10, max_dist=1.0, dof=6, min_pairs=6, eps=None, min_n=1, min_rows=1, since=0,
                    method="point", normals=None):
    """Iterative closest point of B frames against a voxel map: each round takes the origin from the current poses (voxel_align_origin),
    then the sums (voxel_map_align_sums), then the fit (voxel_align_solve), and the loop stops when the step of every frame that was
    fitted is below eps = (radians, cells), or after `iterations` rounds.  poses float64 [B,12] or [B,4]: the start - voxel_map_match's
    best, or the odometry's.  -> {"poses": float64 [B,12], "ok": bool [B] - the last round fitted the frame -, "sums": the last round's
    int64 [B,19], "rounds": the rounds used, "pairs": int64 [rounds,B], "rms": float64 [rounds,B] = sqrt(D / W) size / 256, the pairs'
    root mean square distance in metres as each round found it}.  A frame with fewer than min_pairs pairs in a round keeps its pose in
    that round.  The map is not changed.  eps None: (1e-5, 1 / 256), and VOXEL_ALIGN_PLANE_EPS for the planes.
    method="plane" (group (Y)) fits point-to-plane residuals instead - voxel_map_align_plane_sums and voxel_align_solve_plane, which let a
    row slide along the plane it lies on: "sums" is int64 [B,32], "pairs" counts the plane pairs and "rms" is the root mean square distance
    to the planes.  normals: what voxel_map_normals returned for this map (None: fitted here, with its defaults and these filters)."""
    voxel_align_max_d2(max_dist)
    if method not in VOXEL_ALIGN_METHODS:
        raise ValueError("method must be 'point' or 'plane', got %r" % (method,))
    xyz, n, counts, p, _ = _voxel_align_setup(map_state, xyz, n, counts, poses, np.zeros((np.asarray(xyz).shape[0], 3), np.int64))
    if method == "point":
        if normals is not None:
            raise ValueError("normals go with method='plane'")
        sums_of = lambda cur, origin: voxel_map_align_sums(map_state, xyz, n, counts, cur, origin, max_dist, min_n, min_rows, since)["sums"]  # noqa: E731
        return voxel_align_loop(sums_of, map_state["params"], p, iterations, dof, min_pairs, (1e-5, 1.0 / 256) if eps is None else eps)
    if normals is None:
        normals = voxel_map_normals(map_state, voxel_normal_dirs(), min_n=min_n, min_rows=min_rows, since=since)
    normal, dirs = normals["normal"], normals["dirs"]
    sums_of = lambda cur, origin: voxel_map_align_plane_sums(map_state, xyz, n, counts, cur, origin, normal, dirs, max_dist, min_n, min_rows, since)["sums"]  # noqa: E731
    return voxel_align_loop(sums_of, map_state["params"], p, iterations, dof, min_pairs, VOXEL_ALIGN_PLANE_EPS if eps is None else eps, voxel_align_plane_solver(dirs))


VOXEL_NORMAL_DIRS_MAX = 4096
VOXEL_NORMAL_FIT = ("N", "lam1", "lam2", "lam3")
VOXEL_NORMAL_COUNTS = ("members", "enough", "normals", "zero")
VOXEL_PLANE_SUMS = ("inside", "pairs", "planes", "W", "E") + tuple("g%d" % i for i in range(6)) + tuple("A%d%d" % (i, j) for i in range(6) for j in range(i, 6))  # the 32 words
VOXEL_PLANE_LEVER_SHIFT = 4  # the lever arm (p - o) >> 4, in 1/16 of a cell


def voxel_normal_dirs(m=16, radius=127):
    """The table of candidate directions, int8 [K,4] with K = 2 m^2 + 1 (513 for m = 16): the integer points with |x| + |y| + |z| = m, of
    each antipodal pair the one whose first non-zero of (z, y, x) is positive, sorted by (z, y, x), each scaled to rint(radius v / |v|);
    the fourth byte is 0.  m in 1 .. 45, radius in 1 .. 127 (ValueError).  The norms are nearly one: for m = 16 and radius 127 the squared
    norm s lies in 15972 .. 16265."""
    for v, what, most in ((m, "m", 45), (radius, "radius", 127)):
        if isinstance(v, (bool, np.bool_)) or int(v) != v or not 1 <= v <= most:
            raise ValueError("%s must be an integer in 1 .. %d, got %r" % (what, most, v))
    m, pts = int(m), []
    for z in range(-m, m + 1):
        for y in range(-(m - abs(z)), m - abs(z) + 1):
            for x in {m - abs(z) - abs(y), -(m - abs(z) - abs(y))}:
                if next((c for c in (z, y, x) if c != 0), 0) > 0:
                    pts.append((z, y, x))
    v = np.array(sorted(pts), np.float64)[:, ::-1]  # (x, y, z), in the order of (z, y, x)
    out = np.zeros((len(v), 4), np.int8)
    out[:, :3] = np.rint(float(radius) * v / np.sqrt((v * v).sum(1))[:, None]).astype(np.int8)
    return out


def voxel_normal_vectors(dirs, normal):
    """float64 [.,3]: the unit vector of every direction index in `normal` (any shape), (0, 0, 0) for -1 and for a zero direction."""
    d = _voxel_normal_table(dirs)[:, :3].astype(np.float64)
    length = np.sqrt((d * d).sum(1))
    unit = np.concatenate([d / np.where(length > 0, length, 1.0)[:, None], np.zeros((1, 3))])
    at = np.asarray(normal).astype(np.int64)
    return unit[np.where((at >= 0) & (at < len(d)), at, len(d))]


def _voxel_normal_table(dirs):
    d = np.asarray(dirs)
    if d.dtype != np.int8 or d.ndim != 2 or d.shape[1] != 4 or not 1 <= d.shape[0] <= VOXEL_NORMAL_DIRS_MAX:
        raise ValueError("dirs must be int8 [K,4] with 1 <= K <= 4096, got %s %s" % (d.dtype, d.shape))
    return d


def _voxel_normal_words(min_nb, flat, wide):
    for v, what, lo, hi in ((min_nb, "min_nb", 3, 27), (flat, "flat", 0, 256), (wide, "wide", 0, 256)):
        if isinstance(v, (bool, np.bool_)) or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    return int(min_nb), int(flat), int(wide)


def _voxel_normal_verdict(N, T, lam1, lam3, min_nb, flat, wide):
    lam2 = T - lam1 - lam3
    return lam2, (N >= min_nb) & (lam2 > 0) & (256 * lam3 <= flat * lam2) & (256 * lam2 >= wide * lam1)


def voxel_map_normals(map_state, dirs, min_nb=5, flat=64, wide=16, min_n=1, min_rows=1, since=0):
    """The definition of the voxels' surface normals, include/stereo_vision_hip.h (Y1), in numpy: per voxel the best of a fixed table of
    integer directions under an exact integer criterion.  -> {"normal": int32 [E] - per entry of the map in ascending key, the index of
    the direction or -1 -, "fit": int64 [E,4] = N, lam1, lam2, lam3 of every member, zeros elsewhere, "counts": int64 [4] = members,
    members with N >= min_nb, normals given, 0, "key": int64 [E], the entries' keys, "dirs": the table}.

      members     the voxels that pass voxel_map_rows' filters with n >= max(min_n, 1); a tombstone is neither a member nor a neighbour.
      position    q_k = 256 cell_k + ((S_k // n) >> 8), voxel_map_align_sums' and the flatten's, in 1/256 of a cell.
      neighbours  of member v the members in the up to 27 cells c + d, d in {-1, 0, 1}^3, inside the box - a cell is tested against the
                  box before its key is formed -, v among them.  e = q_j - q_v, |e_k| <= 511; N their number, s1 = sum e, s2 = sum e e^T,
                  C = N s2 - s1 s1^T (|C_ij| < 2^28), T = C00 + C11 + C22.
      directions  dirs int8 [K,4], 1 <= K <= 4096, the fourth byte ignored; s_k = |d_k|^2, Q_k = d_k^T C d_k.  k is flatter than j iff
                  Q_k s_j < Q_j s_k, or both are equal and k < j; a direction with s_k = 0 is never chosen.  best the flattest, worst the
                  one with the largest Q / s, ties to the lower index.  lam3 = Q_best // s_best, lam1 = Q_worst // s_worst (both 0 for a
                  table of zero vectors), lam2 = T - lam1 - lam3.
      verdict     normal = best where N >= min_nb, lam2 > 0, 256 lam3 <= flat lam2 and 256 lam2 >= wide lam1, else -1: a pole or an
                  edge has one wide axis and gets none, a blob neither.  min_nb in 3 .. 27, flat and wide in 0 .. 256 (ValueError).
    An overflowed map: every normal -1, fit and counts 0."""
    min_nb, flat, wide = _voxel_normal_words(min_nb, flat, wide)
    d = _voxel_normal_table(dirs)
    order = np.argsort(map_state["key"], kind="stable")
    E = len(order)
    out = {"normal": np.full(E, -1, np.int32), "fit": np.zeros((E, 4), np.int64), "counts": np.zeros(4, np.int64), "key": map_state["key"][order].astype(np.int64), "dirs": d}
    if map_state["overflowed"] or not E:
        return out
    sel = ((map_state["n"] >= max(min_n, 1)) & (map_state["m"] >= min_rows) & (map_state["last_seq"] >= since))[order]
    mkey, mq = _voxel_align_voxels(map_state, min_n, min_rows, since)
    M = len(mkey)
    if not M:
        return out
    cells = np.array(map_state["params"]["cells"], np.int64)
    c = np.stack([mkey & 0xFFFFF, (mkey >> 20) & 0xFFFFF, (mkey >> 40) & 0xFFFFF], -1)
    N, s1, s2 = np.zeros(M, np.int64), np.zeros((M, 3), np.int64), np.zeros((M, 3, 3), np.int64)
    for off in VOXEL_ALIGN_OFFSETS:
        cc = c + np.array(off, np.int64)
        on = ((cc >= 0) & (cc < cells)).all(-1)  # before a key is formed
        key = np.where(on, cc[:, 0] | (cc[:, 1] << 20) | (cc[:, 2] << 40), -2)
        at = np.minimum(np.searchsorted(mkey, key), M - 1)
        hit = on & (mkey[at] == key)
        e = np.where(hit[:, None], mq[at] - mq, 0)
        N += hit
        s1 += e
        s2 += e[:, :, None] * e[:, None, :]
    C = N[:, None, None] * s2 - s1[:, :, None] * s1[:, None, :]
    T = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2]
    dd = d[:, :3].astype(np.int64)
    s = (dd * dd).sum(1)
    best, worst = np.full(M, -1, np.int64), np.full(M, -1, np.int64)
    bQ, bs, wQ, ws = np.zeros(M, np.int64), np.ones(M, np.int64), np.zeros(M, np.int64), np.ones(M, np.int64)
    for k in range(len(dd)):
        if s[k] == 0:
            continue
        Qk = np.einsum("i,mij,j->m", dd[k], C, dd[k])
        flatter = (best < 0) | (Qk * bs < bQ * s[k])  # strict: a tie stays with the lower index
        best[flatter], bQ[flatter], bs[flatter] = k, Qk[flatter], s[k]
        wider = (worst < 0) | (Qk * ws > wQ * s[k])
        worst[wider], wQ[wider], ws[wider] = k, Qk[wider], s[k]
    lam3, lam1 = bQ // bs, wQ // ws
    lam2, given = _voxel_normal_verdict(N, T, lam1, lam3, min_nb, flat, wide)
    given &= best >= 0
    out["normal"][sel] = np.where(given, best, -1)
    out["fit"][sel] = np.stack([N, lam1, lam2, lam3], -1)
    out["counts"][:3] = M, int((N >= min_nb).sum()), int(given.sum())
    return out


def voxel_map_normals_brute(map_state, dirs, min_nb=5, flat=64, wide=16, min_n=1, min_rows=1, since=0):
    """voxel_map_normals by a Python loop per voxel over all voxels of the map: Python ints, every comparison of two quotients by
    fractions.Fraction, no key is formed for a neighbour cell and nothing is looked up.  The independent model."""
    from fractions import Fraction
    min_nb, flat, wide = _voxel_normal_words(min_nb, flat, wide)
    d = _voxel_normal_table(dirs)
    order = np.argsort(map_state["key"], kind="stable")
    E = len(order)
    out = {"normal": np.full(E, -1, np.int32), "fit": np.zeros((E, 4), np.int64), "counts": np.zeros(4, np.int64), "key": map_state["key"][order].astype(np.int64), "dirs": d}
    if map_state["overflowed"]:
        return out
    voxels = []  # (entry in ascending key, cell, q) of the members
    for at, i in enumerate(order.tolist()):
        key, vn, S, m, last = int(map_state["key"][i]), int(map_state["n"][i]), map_state["S"][i].tolist(), int(map_state["m"][i]), int(map_state["last_seq"][i])
        if vn >= max(min_n, 1) and m >= min_rows and last >= since:
            cell = [(key >> (20 * k)) & 0xFFFFF for k in range(3)]
            voxels.append((at, cell, [256 * cell[k] + ((S[k] // vn) >> 8) for k in range(3)]))
    table = [[int(v) for v in row[:3]] for row in d.tolist()]
    counts = [len(voxels), 0, 0, 0]
    for at, cell, q in voxels:
        es = [[qj[k] - q[k] for k in range(3)] for _, cj, qj in voxels if all(abs(cj[k] - cell[k]) <= 1 for k in range(3))]
        N = len(es)
        s1 = [sum(e[i] for e in es) for i in range(3)]
        C = [[N * sum(e[i] * e[j] for e in es) - s1[i] * s1[j] for j in range(3)] for i in range(3)]
        T = C[0][0] + C[1][1] + C[2][2]
        best = worst = None
        for k, dk in enumerate(table):
            sk = sum(v * v for v in dk)
            if sk == 0:
                continue
            ratio = Fraction(sum(dk[i] * C[i][j] * dk[j] for i in range(3) for j in range(3)), sk)
            if best is None or ratio < best[0]:
                best = (ratio, k)
            if worst is None or ratio > worst[0]:
                worst = (ratio, k)
        lam3, lam1 = (0, 0) if best is None else (best[0].numerator // best[0].denominator, worst[0].numerator // worst[0].denominator)
        lam2 = T - lam1 - lam3
        given = best is not None and N >= min_nb and lam2 > 0 and 256 * lam3 <= flat * lam2 and 256 * lam2 >= wide * lam1
        out["fit"][at] = (N, lam1, lam2, lam3)
        out["normal"][at] = best[1] if given else -1
        counts[1] += N >= min_nb
        counts[2] += bool(given)
    out["counts"][:] = counts
    return out


def _voxel_plane_setup(map_state, normal, dirs):
    """normal as int64 per entry of the map in ascending key, with the entries' keys and the table's (x, y, z) as int64."""
    d = _voxel_normal_table(dirs)
    nrm = np.asarray(normal)
    if nrm.dtype != np.int32 or nrm.shape != (len(map_state["key"]),):
        raise ValueError("normal must be int32 [%d], one word per entry of the map in ascending key, got %s %s" % (len(map_state["key"]), nrm.dtype, nrm.shape))
    return nrm.astype(np.int64), np.sort(map_state["key"]).astype(np.int64), d[:, :3].astype(np.int64)


def _voxel_plane_words(wt, p, q, nu, o):
    """(b, a [.,6]) of plane pairs as int64: b = nu . (q - p), a = (l x nu, nu) with the lever arm l = (p - o) >> 4."""
    lever = (p - o) >> VOXEL_PLANE_LEVER_SHIFT  # arithmetic: a floor
    return (nu * (q - p)).sum(-1), np.concatenate([np.cross(lever, nu).reshape(-1, 3), nu], -1)


def voxel_map_align_plane_sums(map_state, xyz, n, counts, poses, origin, normal, dirs, max_dist=1.0, min_n=1, min_rows=1, since=0):
    """The definition of include/stereo_vision_hip.h (Y2) in numpy: the sums of one round of point-to-plane alignment.  Rows, world, kept,
    p, candidates, nearest and pair are voxel_map_align_sums', word for word; normal int32, one word per entry of the map in ascending key
    (voxel_map_normals' "normal"; the stage takes it as it is), dirs voxel_map_normals' table.
    -> {"sums": int64 [B,32], "pair_key": int64 [B,cap], "pair_d2": int32 [B,cap], "pair_normal": int32 [B,cap]}.

      plane pair  a pair whose partner's normal is a direction of the table: 0 <= normal < K.  nu = dirs[normal] as integers.
      per pair    l = (p - o) >> 4, an arithmetic shift: the lever arm in 1/16 of a cell.  b = nu . (q - p).  a = (l x nu, nu).
      sums        VOXEL_PLANE_SUMS: inside, pairs - voxel_map_align_sums' -, planes, and over the plane pairs W = sum w, E = sum w b^2,
                  g[6] = sum w a_i b, A[21] = sum w a_i a_j for i <= j row-major; 64-bit two's complement sums.  Contract: sum w
                  (256 |l|max)^2 < 2^63.
      per row     pair_key, pair_d2: voxel_map_align_sums'; pair_normal: the normal word of the nearest candidate where that is a
                  direction of the table, else -1.
    For an overflowed map every sum is 0 and every per-row word is -1."""
    max_d2 = voxel_align_max_d2(max_dist)
    xyz, n, counts, poses, origin = _voxel_align_setup(map_state, xyz, n, counts, poses, origin)
    nrm, ekey, dd = _voxel_plane_setup(map_state, normal, dirs)
    B, cap = xyz.shape[:2]
    out = {"sums": np.zeros((B, 32), np.int64), "pair_key": np.full((B, cap), -1, np.int64), "pair_d2": np.full((B, cap), -1, np.int32), "pair_normal": np.full((B, cap), -1, np.int32)}
    if map_state["overflowed"]:
        return out
    w = map_state["params"]
    cells = np.array(w["cells"], np.int64)
    vkey, vq = _voxel_align_voxels(map_state, min_n, min_rows, since)
    if not len(vkey):  # a stand-in that no cell's key equals
        vkey, vq = np.array([-1], np.int64), np.zeros((1, 3), np.int64)
    iu = np.triu_indices(6)
    for b in range(B):
        rows = int(min(max(int(counts[b]), 0), cap))
        wt = np.ones(rows, np.int64) if n is None else n[b, :rows].astype(np.int64)
        at_row, c, p = _voxel_align_rows(w, xyz[b, :rows].astype(np.float64), wt, poses[b])
        sums = out["sums"][b]
        sums[0] = len(at_row)
        best_d2, best_key, best_q = _voxel_align_nearest(cells, vkey, vq, c, p)
        have = best_key >= 0
        of = nrm[np.minimum(np.searchsorted(ekey, np.where(have, best_key, 0)), max(len(ekey) - 1, 0))] if len(ekey) else np.full(len(have), -1, np.int64)
        of = np.where(have & (of >= 0) & (of < len(dd)), of, -1)
        out["pair_key"][b, at_row[have]] = best_key[have]
        out["pair_d2"][b, at_row[have]] = best_d2[have]
        out["pair_normal"][b, at_row[have]] = of[have]
        pair = have & (best_d2 <= max_d2)
        plane = pair & (of >= 0)
        sums[1], sums[2] = int(pair.sum()), int(plane.sum())
        wp = wt[at_row[plane]]
        with np.errstate(over="ignore"):
            bb, a = _voxel_plane_words(wp, p[plane], best_q[plane], dd[of[plane]], origin[b])
            sums[3], sums[4] = wp.sum(), (wp * bb * bb).sum()
            sums[5:11] = ((wp * bb)[:, None] * a).sum(0)
            sums[11:32] = ((wp[:, None] * a)[:, :, None] * a[:, None, :]).sum(0)[iu]
    return out


def voxel_map_align_plane_sums_brute(map_state, xyz, n, counts, poses, origin, normal, dirs, max_dist=1.0, min_n=1, min_rows=1, since=0):
    """voxel_map_align_plane_sums by voxel_map_align_sums_brute's loop per row over all voxels - Python floats and ints, nothing looked up
    by key - with the plane words added up in Python ints and wrapped to 64 bits at the end.  The independent model."""
    max_d2 = voxel_align_max_d2(max_dist)
    xyz, n, counts, poses, origin = _voxel_align_setup(map_state, xyz, n, counts, poses, origin)
    nrm, ekey, dd = _voxel_plane_setup(map_state, normal, dirs)
    B, cap = xyz.shape[:2]
    out = {"sums": np.zeros((B, 32), np.int64), "pair_key": np.full((B, cap), -1, np.int64), "pair_d2": np.full((B, cap), -1, np.int32), "pair_normal": np.full((B, cap), -1, np.int32)}
    if map_state["overflowed"]:
        return out
    w = map_state["params"]
    by_key = np.argsort(map_state["key"], kind="stable").tolist()
    table = dd.tolist()
    voxels = []
    for at, i in enumerate(by_key):
        key, vn, S, m, last = int(map_state["key"][i]), int(map_state["n"][i]), map_state["S"][i].tolist(), int(map_state["m"][i]), int(map_state["last_seq"][i])
        if vn >= max(min_n, 1) and m >= min_rows and last >= since:
            cell = [(key >> (20 * k)) & 0xFFFFF for k in range(3)]
            voxels.append((key, cell, [256 * cell[k] + ((S[k] // vn) >> 8) for k in range(3)], int(nrm[at])))
    wrap = lambda v: (v + 2 ** 63) % 2 ** 64 - 2 ** 63  # noqa: E731
    for b in range(B):
        pose, o = [float(v) for v in poses[b]], [int(v) for v in origin[b]]
        sums = [0] * 32
        for i in range(max(0, min(int(counts[b]), cap))):
            wt = 1 if n is None else int(n[b, i])
            if wt <= 0:
                continue
            x, y, z = (float(v) for v in xyz[b, i])
            c, p = [], []
            for k in range(3):
                with np.errstate(all="ignore"):
                    Pw = float(((np.float64(pose[3 * k]) * x + np.float64(pose[3 * k + 1]) * y) + np.float64(pose[3 * k + 2]) * z) + np.float64(pose[9 + k]))
                if not (w["lo"][k] < Pw < w["hi"][k]):
                    break
                t = (Pw - w["lo"][k]) / w["size"]
                c.append(min(int(t), w["cells"][k] - 1))
                p.append(256 * c[k] + (min(int((t - float(c[k])) * 65536.0), 65535) >> 8))
            if len(c) < 3:
                continue
            sums[0] += 1
            best = None
            for key, cell, q, of in voxels:
                if all(abs(cell[k] - c[k]) <= 1 for k in range(3)):
                    d2 = sum((p[k] - q[k]) ** 2 for k in range(3))
                    if best is None or (d2, key) < best[:2]:
                        best = (d2, key, q, of)
            if best is None:
                continue
            of = best[3] if 0 <= best[3] < len(table) else -1
            out["pair_key"][b, i], out["pair_d2"][b, i], out["pair_normal"][b, i] = best[1], best[0], of
            if best[0] > max_d2:
                continue
            sums[1] += 1
            if of < 0:
                continue
            nu, q = table[of], best[2]
            lever = [(p[k] - o[k]) >> VOXEL_PLANE_LEVER_SHIFT for k in range(3)]
            bb = sum(nu[k] * (q[k] - p[k]) for k in range(3))
            a = [lever[1] * nu[2] - lever[2] * nu[1], lever[2] * nu[0] - lever[0] * nu[2], lever[0] * nu[1] - lever[1] * nu[0]] + nu
            sums[2] += 1
            sums[3] += wt
            sums[4] += wt * bb * bb
            at = 11
            for i6 in range(6):
                sums[5 + i6] += wt * a[i6] * bb
                for j6 in range(i6, 6):
                    sums[at] += wt * a[i6] * a[j6]
                    at += 1
        out["sums"][b] = [wrap(v) for v in sums]
    return out


def voxel_align_solve_plane(sums, poses, origin, params, dof=6, min_pairs=6, rcond=1e-6):
    """The fit of one point-to-plane round: from the sums of voxel_map_align_plane_sums, the poses they were taken under and their origin
    -> (poses' float64 [B,12], ok bool [B], step float64 [B,2]), as voxel_align_solve.  A (6 x 6, symmetric) and g are made from Python
    integers in double and scaled by sc_i = sqrt(max(A_ii, 1)); x = lstsq(A / sc sc^T, g / sc, rcond) / sc, whose minimum-norm solution
    leaves a direction that nothing constrains alone.  omega = x[:3] / 16 - the lever arm is in 1/16 of a cell, the residual in 1/256 -,
    R_d Rodrigues' rotation of omega, t_d = x[3:] in 1/256 of a cell; dof=4 solves the 4 x 4 system of (omega_z, t).  The new pose and
    step are voxel_align_solve's formulas.  A frame with planes < min_pairs, or without a finite fit, keeps its pose: ok False, step 0."""
    if dof not in (4, 6) or isinstance(dof, bool):
        raise ValueError("dof must be 6 (all of the rotation) or 4 (yaw only), got %r" % (dof,))
    if isinstance(min_pairs, bool) or int(min_pairs) != min_pairs:
        raise ValueError("min_pairs must be an integer, got %r" % (min_pairs,))
    if not (np.isfinite(float(rcond)) and 0 <= float(rcond) < 1):
        raise ValueError("rcond must be in 0 .. 1, got %r" % (rcond,))
    sums, poses = np.asarray(sums), voxel_map_pose_words(poses) if len(np.asarray(poses)) else np.zeros((0, 12))
    B = len(poses)
    origin = np.asarray(origin)
    if sums.shape != (B, 32) or origin.shape != (B, 3):
        raise ValueError("sums must be [%d,32] and origin [%d,3], got %s and %s" % (B, B, sums.shape, origin.shape))
    lo, size = np.array(params["lo"]), np.float64(params["size"])
    out, ok, step = poses.copy(), np.zeros(B, bool), np.zeros((B, 2))
    free = [0, 1, 2, 3, 4, 5] if dof == 6 else [2, 3, 4, 5]
    iu = np.triu_indices(6)
    for b in range(B):
        s = [int(v) for v in sums[b]]
        if s[2] < max(int(min_pairs), 1) or s[3] <= 0:
            continue
        A = np.zeros((6, 6))
        A[iu] = [float(v) for v in s[11:32]]
        A = A + np.triu(A, 1).T
        g = np.array([float(v) for v in s[5:11]])
        A, g = A[np.ix_(free, free)], g[free]
        sc = np.sqrt(np.maximum(np.diag(A), 1.0))
        try:
            x = np.linalg.lstsq(A / np.outer(sc, sc), g / sc, rcond=float(rcond))[0] / sc
        except np.linalg.LinAlgError:
            continue
        full = np.zeros(6)
        full[free] = x
        om, td = full[:3] / 16.0, full[3:]
        angle = float(np.sqrt((om * om).sum()))
        K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
        if angle > 1e-12:
            Rd = np.eye(3) + (np.sin(angle) / angle) * K + ((1.0 - np.cos(angle)) / (angle * angle)) * (K @ K)
        else:
            Rd = np.eye(3) + K
        Xo = lo + origin[b].astype(np.float64) * size / 256.0
        new = np.concatenate([(Rd @ poses[b, :9].reshape(3, 3)).reshape(9), Rd @ (poses[b, 9:] - Xo) + Xo + td * size / 256.0])
        if not np.isfinite(new).all():
            continue
        out[b], ok[b], step[b] = new, True, (angle, float(np.sqrt((td * td).sum())) / 256.0)
    return out, ok, step


def voxel_align_plane_solver(dirs):
    """voxel_align_loop's solver for the plane sums of a table: the 32 words, voxel_align_solve_plane, the planes as the pairs that count,
    and 1 / the table's mean length as the unit of sqrt(E / W)."""
    d = _voxel_normal_table(dirs)[:, :3].astype(np.float64)
    length = np.sqrt((d * d).sum(1))
    mean = float(length[length > 0].mean()) if (length > 0).any() else 1.0
    return dict(words=32, solve=voxel_align_solve_plane, pairs=2, W=3, D=4, unit=1.0 / mean)


FLOW_Z_MIN = 0.1              # metres: a point at or nearer than this in the current camera is dropped
FLOW_R_MAX = 7                # the patch is (2 r + 1)^2, at most 15 x 15
FLOW_CANDIDATES_MAX = 16384   # (2 wx + 1) (2 wy + 1) at most: a candidate's index fits 14 bits beside its 16-bit cost
FLOW_WINDOW_BYTES = 16384     # a point's window of cur, rows padded as flow_window_bytes says, at most: what a wavefront holds in LDS
FLOW_DQ_MAX = 2 ** 20         # a disparity in 1/16 px that makes a point: 1 .. 2^20
FLOW_CENTRE_MAX = 2.0 ** 20   # |c| of a window centre that is kept
FLOW_COST_MAX = 225 * 255     # the largest sum of absolute differences
FLOW_CAPACITY_MAX = 65536     # matches per frame at most: with it every one of flow_pose_sums' words stays below 2^59
FLOW_BATCH_MAX = 65535
FLOW_GATE_MAX = 2 ** 20       # gate_q and dgate_q at most, and what "no gate" stands for: 65536 px
FLOW_PIXEL_MAX = 2.0 ** 30    # |pu|, |pv|, pd of a match that is inside, in 1/16 px
FLOW_J_MAX = 2 ** 20          # a quantised Jacobian entry is clamped to +-this
FLOW_SUMS = ("inside", "inliers", "dinliers", "E", "Ed") + tuple("g%d" % i for i in range(6)) + tuple("A%d%d" % (i, j) for i in range(6) for j in range(i, 6))  # the 32 words
FLOW_GATES = (None, 20, 8, 4, 3)  # px: flow_egomotion's schedule
FLOW_EPS = (2e-5, 2e-4)       # radians and metres: flow_egomotion's default eps.  A round moves a residual by 1/16 px at the least - over
                              # some thousand matches the fit's floor is a few 1e-6 rad and 1e-5 m -, and an inlier set that flickers at the
                              # gate moves the pose by up to 1e-5 rad and 1e-4 m (the synthetic cases of tests/flow_cases.py).


def flow_camera(camera):
    """The words of the temporal matcher from a camera dict (voxel_render_camera's, made from the rig's Q): f, cx, cy as they are, the
    baseline b = 1 / q32 in metres - q32 > 0, and q33, a principal point that differs between the two cameras, is taken as 0 -, and the
    products made once on the host in double: b16 = 16 b, fb = f b, fb16 = f b16.  ValueError for words that are not finite, f <= 0 or
    q32 <= 0."""
    try:
        f, cx, cy, q32 = (float(camera[k]) for k in ("f", "cx", "cy", "q32"))
    except (KeyError, TypeError, ValueError):
        raise ValueError("a camera needs the numbers f, cx, cy and q32")
    if not all(np.isfinite(v) for v in (f, cx, cy, q32)) or not f > 0 or not q32 > 0:
        raise ValueError("the camera's words must be finite with f > 0 and q32 > 0, got f=%r cx=%r cy=%r q32=%r" % (f, cx, cy, q32))
    b = 1.0 / q32
    b16 = 16.0 * b
    w = {"f": f, "cx": cx, "cy": cy, "b": b, "b16": b16, "fb": f * b, "fb16": f * b16}
    if not all(np.isfinite(v) for v in w.values()):
        raise ValueError("the camera's baseline is not finite")
    return w


def flow_window_bytes(r, wx, wy):
    """The bytes a point's window of cur takes on the device: (2 wy + 2 r + 1) rows of an odd number of dwords, (2 wx + 2 r + 1 + 3) // 4
    + 1 made odd - the one dword more is what a patch row that starts at the window's last bytes reads behind it."""
    pitch = (2 * wx + 2 * r + 1 + 3) // 4 + 1
    pitch += 1 - pitch % 2
    return 4 * pitch * (2 * wy + 2 * r + 1)


def flow_words(step=8, r=4, wx=8, wy=8, ratio=230, max_cost=FLOW_COST_MAX, capacity=4096):
    """The words of a flow_match call as a dict of ints, after the checks the C entry makes (ValueError): step >= 1, r in 1 .. 7, wx and wy
    >= 0 with (2 wx + 1) (2 wy + 1) <= 16384 and flow_window_bytes(r, wx, wy) <= 16384, ratio in 0 .. 256, max_cost >= 0, capacity in
    0 .. 65536."""
    w = {}
    for k, v, lo, hi in (("step", step, 1, 2 ** 20), ("r", r, 1, FLOW_R_MAX), ("wx", wx, 0, 8192), ("wy", wy, 0, 8192), ("ratio", ratio, 0, 256),
                         ("max_cost", max_cost, 0, 2 ** 31 - 1), ("capacity", capacity, 0, FLOW_CAPACITY_MAX)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (k, lo, hi, v))
        w[k] = int(v)
    if (2 * w["wx"] + 1) * (2 * w["wy"] + 1) > FLOW_CANDIDATES_MAX:
        raise ValueError("the window has more than %d candidates: wx=%d wy=%d" % (FLOW_CANDIDATES_MAX, w["wx"], w["wy"]))
    if flow_window_bytes(w["r"], w["wx"], w["wy"]) > FLOW_WINDOW_BYTES:
        raise ValueError("the window takes more than %d bytes: r=%d wx=%d wy=%d" % (FLOW_WINDOW_BYTES, w["r"], w["wx"], w["wy"]))
    return w


def _flow_dq(d):
    """floor(16 d + 0.5) in double of float32 disparities, 0 where d is not positive and finite or the value leaves 1 .. 2^20."""
    d = np.asarray(d, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(d * 16.0 + 0.5)
        ok = np.isfinite(d) & (d > 0) & (q >= 1) & (q <= FLOW_DQ_MAX)
    return np.where(ok, q, 0).astype(np.int64)


def _flow_point(cam, u, v, dq):
    """X0 of pixels (u, v) with disparity dq / 16 (arrays of equal shape, dq >= 1), in double, every operation on its own:
    ((u - cx) b16) / dq, ((v - cy) b16) / dq, fb16 / dq."""
    dq = np.asarray(dq, np.float64)
    return ((np.asarray(u, np.float64) - cam["cx"]) * cam["b16"]) / dq, ((np.asarray(v, np.float64) - cam["cy"]) * cam["b16"]) / dq, cam["fb16"] / dq


def _flow_move(pose, x, y, z):
    """Xc = R X0 + t under one pose of twelve doubles, in voxel_map_insert's order: ((R[k,0] x + R[k,1] y) + R[k,2] z) + t[k]."""
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(((pose[3 * k] * x + pose[3 * k + 1] * y) + pose[3 * k + 2] * z) + pose[9 + k] for k in range(3))


def flow_match(prev, cur, d_prev, d_cur, camera, guess=None, step=8, r=4, wx=8, wy=8, ratio=230, max_cost=FLOW_COST_MAX, capacity=4096):
    """Temporal matches of B frame pairs, the definition of include/stereo_vision_hip.h (Z1) in numpy.  prev, cur uint8 [B,H,W]: the
    rectified left gray images of frames k - 1 and k; d_prev float32 [B,H,W]: the disparity of frame k - 1; d_cur float32 [B,H,W] or
    None; camera: voxel_render_camera's dict (flow_camera reads it); guess float64 [B,12] or None: the expected motion, previous camera
    to current camera, Xc = R X0 + t in voxel_map_pose's layout - None is the identity and skips the projection.
      points      the pixels (u0, v0) with u0 % step == 0 and v0 % step == 0, in ascending v0 W + u0, with r <= u0 < W - r, r <= v0 < H - r
                  and d0q = floor(16 d + 0.5) (in double) in 1 .. 2^20 for a positive, finite d = d_prev[v0, u0].
      centre      X0 = (((u0 - cx) b16) / d0q, ((v0 - cy) b16) / d0q, fb16 / d0q), Xc = ((R_k0 x + R_k1 y) + R_k2 z) + t_k; a point with Xc.z
                  <= FLOW_Z_MIN (0.1 m; or NaN) is dropped; c = (floor(((f Xc.x) / Xc.z + cx) + 0.5), floor(((f Xc.y) / Xc.z + cy) + 0.5)), and
                  a point whose c is not within +-2^20 is dropped.  Without a guess c = (u0, v0).
      candidates  (dx, dy) in [-wx, wx] x [-wy, wy] with r <= c.x + dx < W - r and r <= c.y + dy < H - r; cost = the sum of the absolute
                  differences of the (2 r + 1)^2 patch of prev around (u0, v0) and that of cur around c + (dx, dy).
      best        the least cost, among equals the least (dy + wy) (2 wx + 1) + (dx + wx); second: the least cost among the candidates
                  with max(|dx - bdx|, |dy - bdy|) > 1.
      match       a second exists, 256 best < ratio second, best <= max_cost, and the best is not on the rim: not (wx > 0 and |bdx| == wx)
                  and not (wy > 0 and |bdy| == wy).
    -> {"matches": int32 [B,capacity,6] = (u0, v0, d0q, u1, v1, d1q) in point order, (u1, v1) = c + best, d1q = floor(16 d_cur[v1, u1] + 0.5)
    where that is in 1 .. 2^20 for a positive finite d_cur, else -1; "cost": int32 [B,capacity,2] = (best, second); "counts": int32 [B], -1
    for a frame with more matches than capacity, whose rows are the first `capacity` of them}.  Rows at and behind a frame's count hold
    -1."""
    w = flow_words(step, r, wx, wy, ratio, max_cost, capacity)
    cam = flow_camera(camera)
    prev, cur = np.asarray(prev), np.asarray(cur)
    if prev.dtype != np.uint8 or prev.ndim != 3 or cur.dtype != np.uint8 or cur.shape != prev.shape:
        raise ValueError("prev and cur must be uint8 [B,H,W] of one shape, got %s %s and %s %s" % (prev.dtype, prev.shape, cur.dtype, cur.shape))
    B, H, W = prev.shape
    if B > FLOW_BATCH_MAX or not (1 <= W <= 8192 and 1 <= H <= 8192):
        raise ValueError("at most 65535 frames of at most 8192 x 8192, got %s" % (prev.shape,))
    d_prev = np.asarray(d_prev)
    if d_prev.dtype != np.float32 or d_prev.shape != prev.shape or (d_cur is not None and (np.asarray(d_cur).dtype != np.float32 or np.asarray(d_cur).shape != prev.shape)):
        raise ValueError("d_prev (and d_cur) must be float32 %s" % (prev.shape,))
    if guess is not None:
        guess = np.asarray(guess, np.float64)
        if guess.shape != (B, 12):
            raise ValueError("guess must be float64 [%d,12], got %s" % (B, guess.shape))
    r, wx, wy, cap = w["r"], w["wx"], w["wy"], w["capacity"]
    nwx, nwy, side = 2 * wx + 1, 2 * wy + 1, 2 * r + 1
    BIG = 1 << 30
    matches, cost, counts = np.full((B, cap, 6), -1, np.int32), np.full((B, cap, 2), -1, np.int32), np.zeros(B, np.int32)
    vs, us = np.meshgrid(np.arange(0, H, w["step"]), np.arange(0, W, w["step"]), indexing="ij")
    vs, us = vs.ravel(), us.ravel()
    for b in range(B):
        dq0 = _flow_dq(d_prev[b])
        dq1 = None if d_cur is None else _flow_dq(np.asarray(d_cur)[b])
        q = dq0[vs, us]
        keep = (q > 0) & (us >= r) & (us < W - r) & (vs >= r) & (vs < H - r)
        cxs, cys = us.astype(np.float64), vs.astype(np.float64)
        if guess is not None:
            x, y, z = _flow_point(cam, us, vs, np.maximum(q, 1))
            X = _flow_move(guess[b], x, y, z)
            with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
                keep &= X[2] > FLOW_Z_MIN
                zs = np.where(keep, X[2], 1.0)
                cxs, cys = np.floor(((cam["f"] * X[0]) / zs + cam["cx"]) + 0.5), np.floor(((cam["f"] * X[1]) / zs + cam["cy"]) + 0.5)
                keep &= (np.abs(cxs) <= FLOW_CENTRE_MAX) & (np.abs(cys) <= FLOW_CENTRE_MAX)  # false for NaN
        found = 0
        P, C = prev[b].astype(np.int32), cur[b].astype(np.int32)
        for i in np.flatnonzero(keep):
            u0, v0, ccx, ccy = int(us[i]), int(vs[i]), int(cxs[i]), int(cys[i])
            x_lo, x_hi, y_lo, y_hi = max(ccx - wx, r), min(ccx + wx, W - r - 1), max(ccy - wy, r), min(ccy + wy, H - r - 1)
            if x_lo > x_hi or y_lo > y_hi:
                continue
            view = np.lib.stride_tricks.sliding_window_view(C[y_lo - r:y_hi + r + 1, x_lo - r:x_hi + r + 1], (side, side))
            full = np.full((nwy, nwx), BIG, np.int64)
            full[y_lo - ccy + wy:y_hi - ccy + wy + 1, x_lo - ccx + wx:x_hi - ccx + wx + 1] = np.abs(view - P[v0 - r:v0 + r + 1, u0 - r:u0 + r + 1]).sum((2, 3))
            at = int(full.argmin())  # the first of equals
            by, bx = divmod(at, nwx)
            best = int(full[by, bx])
            full[max(by - 1, 0):by + 2, max(bx - 1, 0):bx + 2] = BIG
            second = int(full.min())
            if second >= BIG or not 256 * best < w["ratio"] * second or best > w["max_cost"]:
                continue
            if (wx > 0 and abs(bx - wx) == wx) or (wy > 0 and abs(by - wy) == wy):
                continue
            if found < cap:
                u1, v1 = ccx + bx - wx, ccy + by - wy
                d1 = -1 if dq1 is None or dq1[v1, u1] == 0 else int(dq1[v1, u1])
                matches[b, found], cost[b, found] = (u0, v0, int(q[i]), u1, v1, d1), (best, second)
            found += 1
        counts[b] = found if found <= cap else -1
    return {"matches": matches, "cost": cost, "counts": counts}


def _flow_gates(gate_q, dgate_q):
    out = []
    for v, what in ((gate_q, "gate_q"), (dgate_q, "dgate_q")):
        v = FLOW_GATE_MAX if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= FLOW_GATE_MAX:
            raise ValueError("%s must be an integer in 0 .. 2^20 (1/16 px) or None, got %r" % (what, v))
        out.append(int(v))
    return out


def _flow_sums_setup(matches, counts, poses):
    matches, counts = np.asarray(matches), np.asarray(counts)
    if matches.dtype != np.int32 or matches.ndim != 3 or matches.shape[2] != 6 or matches.shape[1] > FLOW_CAPACITY_MAX or matches.shape[0] > FLOW_BATCH_MAX:
        raise ValueError("matches must be int32 [B,capacity,6] with capacity <= 65536 and B <= 65535, got %s %s" % (matches.dtype, matches.shape))
    B = matches.shape[0]
    if counts.dtype != np.int32 or counts.shape != (B,):
        raise ValueError("counts must be int32 [%d], got %s %s" % (B, counts.dtype, counts.shape))
    poses = np.asarray(poses, np.float64)
    if poses.shape != (B, 12):
        raise ValueError("poses must be float64 [%d,12], got %s" % (B, poses.shape))
    return matches, counts, poses


def _flow_q(v, lim):
    """floor(v + 0.5) of doubles, clamped to +-lim, as int64."""
    return np.clip(np.floor(v + 0.5), -lim, lim).astype(np.int64)


def flow_pose_sums(matches, counts, camera, poses, gate_q=None, dgate_q=None):
    """The sums of one Gauss-Newton round of the egomotion fit, the definition of include/stereo_vision_hip.h (Z2) in numpy.  matches int32
    [B,capacity,6] and counts int32 [B] as flow_match gives them (a count of -1 or 0 gives sums of 0; a count beyond the capacity counts as
    the capacity), poses float64 [B,12]: previous camera to current camera, gate_q and dgate_q in 1/16 px, 0 .. 2^20, None: 2^20.
      per match   d0q in 1 .. 2^20, else it is skipped.  X0 as in flow_match, Xc = R X0 + t in its order, (x, y, z) = Xc.  fz = f / z,
                  xz = x / z, yz = y / z, bz = fb / z.  pu = floor(16 (f xz + cx) + 0.5), pv = floor(16 (f yz + cy) + 0.5), pd = floor(16 bz +
                  0.5), as doubles.  inside: z > FLOW_Z_MIN and |pu|, |pv|, |pd| <= 2^30 (false for NaN).
      residuals   ru = 16 u1 - pu, rv = 16 v1 - pv, rd = d1q - pd, integers.  inlier: inside, |ru| <= gate_q, |rv| <= gate_q and ru^2 + rv^2 <=
                  gate_q^2; d-inlier: an inlier with d1q > 0 and |rd| <= dgate_q.
      Jacobian    with respect to (t, omega) of Xc' = exp(omega) Xc + t: a = fz xz, Ju = (fz, 0, -a, -(a y), f (1 + xz xz), -(f yz)); c = fz yz,
                  Jv = (0, fz, -c, -(f (1 + yz yz)), a y, f xz); e = bz / z, Jd = (0, 0, -e, -(e y), e x, 0); every entry quantised as
                  clamp(floor(16 J + 0.5), +-2^20).
      sums        int64 [B,32], FLOW_SUMS: inside, inliers, dinliers, E = sum ru^2 + rv^2, Ed = sum rd^2, g[6] = sum Jq r, A[21] = sum Jq_i Jq_j,
                  the upper triangle row-major - the u and v rows of the inliers, the d rows of the d-inliers.  Every word stays below 2^59.
    -> int64 [B,32]."""
    gate_q, dgate_q = _flow_gates(gate_q, dgate_q)
    cam = flow_camera(camera)
    matches, counts, poses = _flow_sums_setup(matches, counts, poses)
    B, cap = matches.shape[:2]
    sums = np.zeros((B, 32), np.int64)
    iu = np.triu_indices(6)
    for b in range(B):
        n = min(int(counts[b]), cap)
        if n <= 0:
            continue
        m = matches[b, :n].astype(np.int64)
        u0, v0, d0, u1, v1, d1 = (m[:, k] for k in range(6))
        live = (d0 >= 1) & (d0 <= FLOW_DQ_MAX)
        x0, y0, z0 = _flow_point(cam, u0, v0, np.where(live, d0, 1))
        x, y, z = _flow_move(poses[b], x0, y0, z0)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            live &= z > FLOW_Z_MIN
            z = np.where(live, z, 1.0)
            fz, xz, yz, bz = cam["f"] / z, x / z, y / z, cam["fb"] / z
            pu, pv, pd = np.floor(16.0 * (cam["f"] * xz + cam["cx"]) + 0.5), np.floor(16.0 * (cam["f"] * yz + cam["cy"]) + 0.5), np.floor(16.0 * bz + 0.5)
            inside = live & (np.abs(pu) <= FLOW_PIXEL_MAX) & (np.abs(pv) <= FLOW_PIXEL_MAX) & (np.abs(pd) <= FLOW_PIXEL_MAX)
            zero = np.zeros_like(z)
            a, c, e = fz * xz, fz * yz, bz / z
            J = np.stack([np.stack([fz, zero, -a, -(a * y), cam["f"] * (1.0 + xz * xz), -(cam["f"] * yz)], -1),
                          np.stack([zero, fz, -c, -(cam["f"] * (1.0 + yz * yz)), a * y, cam["f"] * xz], -1),
                          np.stack([zero, zero, -e, -(e * y), e * x, zero], -1)], 1)  # [n,3,6]
            J = np.where(inside[:, None, None], J, 0.0)
            Jq = _flow_q(16.0 * J, FLOW_J_MAX)
        pu, pv, pd = (np.where(inside, p, 0.0).astype(np.int64) for p in (pu, pv, pd))
        ru, rv, rd = 16 * u1 - pu, 16 * v1 - pv, d1 - pd
        inl = inside & (np.abs(ru) <= gate_q) & (np.abs(rv) <= gate_q)
        ru, rv = np.where(inl, ru, 0), np.where(inl, rv, 0)
        inl &= ru * ru + rv * rv <= gate_q * gate_q
        dinl = inl & (d1 > 0) & (np.abs(rd) <= dgate_q)
        res = np.stack([np.where(inl, ru, 0), np.where(inl, rv, 0), np.where(dinl, rd, 0)], 1)  # [n,3]
        Jq = Jq * np.stack([inl, inl, dinl], 1)[:, :, None]
        sums[b, 0], sums[b, 1], sums[b, 2] = inside.sum(), inl.sum(), dinl.sum()
        sums[b, 3], sums[b, 4] = (res[:, 0] ** 2 + res[:, 1] ** 2).sum(), (res[:, 2] ** 2).sum()
        sums[b, 5:11] = (Jq * res[:, :, None]).sum((0, 1))
        sums[b, 11:] = np.einsum("nki,nkj->ij", Jq, Jq)[iu]
    return sums


def flow_pose_sums_brute(matches, counts, camera, poses, gate_q=None, dgate_q=None):
    """flow_pose_sums match by match: Python floats in the stated order in front of the rounding, Python integers behind it."""
    import math
    gate_q, dgate_q = _flow_gates(gate_q, dgate_q)
    cam = flow_camera(camera)
    matches, counts, poses = _flow_sums_setup(matches, counts, poses)
    f, cx, cy, b16, fb, fb16 = (cam[k] for k in ("f", "cx", "cy", "b16", "fb", "fb16"))
    B, cap = matches.shape[:2]
    out = np.zeros((B, 32), np.int64)

    def rnd(v):
        return math.floor(v + 0.5)

    for b in range(B):
        s = [0] * 32
        p = [float(v) for v in poses[b]]
        for i in range(max(min(int(counts[b]), cap), 0)):
            u0, v0, d0, u1, v1, d1 = (int(v) for v in matches[b, i])
            if not 1 <= d0 <= FLOW_DQ_MAX:
                continue
            X0 = (((u0 - cx) * b16) / d0, ((v0 - cy) * b16) / d0, fb16 / d0)
            x, y, z = (((p[3 * k] * X0[0] + p[3 * k + 1] * X0[1]) + p[3 * k + 2] * X0[2]) + p[9 + k] for k in range(3))
            if not z > FLOW_Z_MIN:
                continue
            fz, xz, yz, bz = f / z, x / z, y / z, fb / z
            pred = (16.0 * (f * xz + cx) + 0.5, 16.0 * (f * yz + cy) + 0.5, 16.0 * bz + 0.5)
            if not all(math.isfinite(v) and abs(math.floor(v)) <= FLOW_PIXEL_MAX for v in pred):
                continue
            pu, pv, pd = (math.floor(v) for v in pred)
            s[0] += 1
            ru, rv, rd = 16 * u1 - pu, 16 * v1 - pv, d1 - pd
            if ru * ru + rv * rv > gate_q * gate_q:
                continue
            s[1] += 1
            a, c, e = fz * xz, fz * yz, bz / z
            rows = [((fz, 0.0, -a, -(a * y), f * (1.0 + xz * xz), -(f * yz)), ru), ((0.0, fz, -c, -(f * (1.0 + yz * yz)), a * y, f * xz), rv)]
            s[3] += ru * ru + rv * rv
            if d1 > 0 and abs(rd) <= dgate_q:
                s[2] += 1
                s[4] += rd * rd
                rows.append(((0.0, 0.0, -e, -(e * y), e * x, 0.0), rd))
            for J, res in rows:
                Jq = [max(-FLOW_J_MAX, min(FLOW_J_MAX, rnd(16.0 * v))) for v in J]
                at = 11
                for i6 in range(6):
                    s[5 + i6] += Jq[i6] * res
                    for j6 in range(i6, 6):
                        s[at] += Jq[i6] * Jq[j6]
                        at += 1
        out[b] = s
    return out


def _flow_exp(om):
    """Rodrigues' rotation of the vector om (radians), as voxel_align_solve_plane makes it."""
    angle = float(np.sqrt((om * om).sum()))
    K = np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]], [-om[1], om[0], 0.0]])
    if angle > 1e-12:
        return np.eye(3) + (np.sin(angle) / angle) * K + ((1.0 - np.cos(angle)) / (angle * angle)) * (K @ K), angle
    return np.eye(3) + K, angle


def flow_solve(sums, poses, min_inliers=12, rcond=1e-6):
    """The fit of one round: from flow_pose_sums' words and the poses they were taken under -> (poses' float64 [B,12], ok bool [B], step
    float64 [B,2] = (radians, metres)).  A (6 x 6, symmetric) and g from Python integers in double, scaled by sc_i = sqrt(max(A_ii, 1));
    delta = lstsq(A / sc sc^T, g / sc, rcond) / sc - the minimum-norm solution, as voxel_align_solve_plane's; the residuals' and the
    Jacobian's factors of 16 cancel, so delta = (t_d in metres, omega in radians).  R' = exp(omega) R, t' = exp(omega) t + t_d.  A frame
    with inliers < min_inliers, or without a finite fit, keeps its pose: ok False, step 0."""
    if isinstance(min_inliers, bool) or int(min_inliers) != min_inliers:
        raise ValueError("min_inliers must be an integer, got %r" % (min_inliers,))
    sums, poses = np.asarray(sums), np.asarray(poses, np.float64)
    B = len(poses)
    if sums.shape != (B, 32) or poses.shape != (B, 12):
        raise ValueError("sums must be [B,32] and poses [B,12], got %s and %s" % (sums.shape, poses.shape))
    out, ok, step = poses.copy(), np.zeros(B, bool), np.zeros((B, 2))
    iu = np.triu_indices(6)
    for b in range(B):
        s = [int(v) for v in sums[b]]
        if s[1] < max(int(min_inliers), 1):
            continue
        A = np.zeros((6, 6))
        A[iu] = [float(v) for v in s[11:32]]
        A = A + np.triu(A, 1).T
        g = np.array([float(v) for v in s[5:11]])
        sc = np.sqrt(np.maximum(np.diag(A), 1.0))
        try:
            x = np.linalg.lstsq(A / np.outer(sc, sc), g / sc, rcond=float(rcond))[0] / sc
        except np.linalg.LinAlgError:
            continue
        td, om = x[:3], x[3:]
        if not np.isfinite(x).all():
            continue
        Rd, angle = _flow_exp(om)
        new = np.concatenate([(Rd @ poses[b, :9].reshape(3, 3)).reshape(9), Rd @ poses[b, 9:] + td])
        if not np.isfinite(new).all():
            continue
        out[b], ok[b], step[b] = new, True, (angle, float(np.sqrt((td * td).sum())))
    return out, ok, step


def flow_identity(B):
    """float64 [B,12]: B identity motions."""
    return np.tile(np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0]), (int(B), 1))


def flow_loop(sums_of, start, gates=FLOW_GATES, dgate=2.0, iterations=10, eps=None, min_inliers=12):
    """flow_egomotion's loop around any source of sums - sums_of(poses [B,12], gate_q, dgate_q) -> int64 [B,32]: the numpy definition's or
    the device's, read back.  Everything else is host numpy, the same for both."""
    eps = FLOW_EPS if eps is None else eps
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 0:
        raise ValueError("iterations must be an integer >= 0, got %r" % (iterations,))
    if len(eps) != 2 or not all(np.isfinite(float(e)) and float(e) >= 0 for e in eps):
        raise ValueError("eps must be two finite numbers >= 0: radians and metres, got %r" % (eps,))
    gates = tuple(gates)
    if not gates or not all(g is None or (np.isfinite(float(g)) and 0 <= float(g) <= 65536) for g in gates) or not 0 <= float(dgate) <= 65536:
        raise ValueError("gates must be pixels in 0 .. 65536 or None, at least one, and dgate pixels, got %r and %r" % (gates, dgate))
    gates_q = [None if g is None else int(np.floor(16.0 * float(g) + 0.5)) for g in gates]
    dgate_q = int(np.floor(16.0 * float(dgate) + 0.5))
    poses = np.ascontiguousarray(np.asarray(start, np.float64))
    B = len(poses)
    sums, ok = np.zeros((B, 32), np.int64), np.zeros(B, bool)
    inliers, rms, rounds = [], [], 0
    for i in range(int(iterations)):
        sums = np.ascontiguousarray(sums_of(poses, gates_q[min(i, len(gates_q) - 1)], dgate_q), np.int64)
        poses, ok, step = flow_solve(sums, poses, min_inliers)
        rounds += 1
        n, E = sums[:, 1].astype(np.float64), sums[:, 3].astype(np.float64)
        inliers.append(sums[:, 1].copy())
        rms.append(np.where(n > 0, np.sqrt(E / np.maximum(n, 1.0)) / 16.0, 0.0))
        if i >= len(gates_q) - 1 and ((step[ok, 0] < eps[0]) & (step[ok, 1] < eps[1])).all():
            break
    return {"poses": poses, "ok": ok, "rounds": rounds, "inliers": np.array(inliers, np.int64).reshape(rounds, B), "rms_px": np.array(rms, np.float64).reshape(rounds, B),
            "sums": sums}


def flow_egomotion(matches, counts, camera, start=None, gates=FLOW_GATES, dgate=2.0, iterations=10, eps=None, min_inliers=12):
    """The camera's motion between two frames from their temporal matches: a gated Gauss-Newton loop over flow_pose_sums and flow_solve.
    start float64 [B,12] or None (the identity): previous camera to current camera.  Round i gates the reprojection error at
    gates[min(i, len - 1)] pixels (None: no gate) and the disparity's at dgate pixels; the loop stops once the schedule is through and
    every fitted frame's step is below eps = (radians, metres) - None: FLOW_EPS -, or after `iterations` rounds.  -> {"poses": float64
    [B,12], "ok": bool [B] - the last round fitted the frame -, "rounds", "inliers": int64 [rounds,B], "rms_px": float64 [rounds,B] = sqrt(E /
    inliers) / 16 as each round found them, "sums": the last round's int64 [B,32]}.  The inliers of the result are those of the last round's
    sums: counted under the pose that round started from."""
    matches, counts = np.asarray(matches), np.asarray(counts)
    start = flow_identity(matches.shape[0]) if start is None else start
    _flow_sums_setup(matches, counts, start)
    return flow_loop(lambda poses, gate_q, dgate_q: flow_pose_sums(matches, counts, camera, poses, gate_q, dgate_q), start, gates, dgate, iterations, eps, min_inliers)


def flow_chain(rel, start=None, XR=None, XT=None, ok=None):
    """The poses of B + 1 frames from B motions between them: float64 [B+1,12], frame to world in voxel_map_pose's layout - what update(),
    align() and --poses take.  rel float64 [B,12]: motion k carries the camera of frame k into that of frame k + 1 (Xc' = R Xc + t,
    flow_egomotion's); start: the pose of frame 0 ([12]; None: the identity); XR, XT: the rig's transform, camera to frame (Pf = XR Pc + XT;
    None: the identity, zero); ok bool [B] or None: a motion that is not ok is replaced by the one before it, the first such by the
    identity.  W_k = W_{k-1} M T_k^-1 M^-1 with M = (XR | XT) and T^-1 = (R^T | -(R^T t)): the inverse is the transpose, R and XR must be
    rotations.  Every product of two rigid motions is made on its own, as voxel_render_cams makes them: (Ra | ta) (Rb | tb) = (Ra Rb | Ra
    tb + ta) with C[i,j] = (Ra[i,0] Rb[0,j] + Ra[i,1] Rb[1,j]) + Ra[i,2] Rb[2,j] and o[i] = ((Ra[i,0] tb[0] + Ra[i,1] tb[1]) + Ra[i,2] tb[2]) +
    ta[i], taken from the left: ((W M) T^-1) M^-1."""
    rel = np.asarray(rel, np.float64).reshape(-1, 12)
    B = len(rel)
    ok = np.ones(B, bool) if ok is None else np.asarray(ok, bool).reshape(B)
    XR = np.eye(3) if XR is None else np.asarray(XR, np.float64).reshape(3, 3)
    XT = np.zeros(3) if XT is None else np.asarray(XT, np.float64).reshape(3)
    start = flow_identity(1)[0] if start is None else np.asarray(start, np.float64).reshape(12)

    def mul(Ra, ta, Rb, tb):
        C = np.array([[(Ra[i, 0] * Rb[0, j] + Ra[i, 1] * Rb[1, j]) + Ra[i, 2] * Rb[2, j] for j in range(3)] for i in range(3)])
        o = np.array([((Ra[i, 0] * tb[0] + Ra[i, 1] * tb[1]) + Ra[i, 2] * tb[2]) + ta[i] for i in range(3)])
        return C, o

    def inv(R, t):
        Rt = R.T
        return Rt, np.array([-((Rt[k, 0] * t[0] + Rt[k, 1] * t[1]) + Rt[k, 2] * t[2]) for k in range(3)])

    Mi = inv(XR, XT)
    out = [start.copy()]
    last = flow_identity(1)[0]
    for k in range(B):
        last = rel[k] if ok[k] else last
        W = (out[-1][:9].reshape(3, 3), out[-1][9:])
        W = mul(*W, XR, XT)
        W = mul(*W, *inv(last[:9].reshape(3, 3), last[9:]))
        W = mul(*W, *Mi)
        out.append(np.concatenate([W[0].reshape(9), W[1]]))
    return np.ascontiguousarray(np.array(out))


FLOW_ODOMETRY = dict(step=8, r=4, wx=8, wy=8, ratio=230, max_cost=FLOW_COST_MAX, capacity=8192, cold=(64, 24), first=None, gates=FLOW_GATES, dgate=2.0, iterations=10,
                     eps=None, min_inliers=12)  # the words of flow_odometry and StereoRig.odometry, and their defaults


def flow_odometry_spec(**spec):
    """FLOW_ODOMETRY with the caller's words in place of the defaults; ValueError for a word it does not have."""
    unknown = sorted(set(spec) - set(FLOW_ODOMETRY))
    if unknown:
        raise ValueError("unknown words %s: the odometry takes %s" % (unknown, sorted(FLOW_ODOMETRY)))
    s = dict(FLOW_ODOMETRY, **spec)
    if len(tuple(s["cold"])) != 2:
        raise ValueError("cold must be (wx, wy), got %r" % (s["cold"],))
    return s


def flow_odometry(match_of, ego_of, pairs, guess="velocity", **spec):
    """The motions of `pairs` consecutive frame pairs, pair k being frames (k, k + 1) - what StereoRig.odometry runs with device
    callables and the tests with flow_match and flow_egomotion.  match_of(lo, hi, guess [hi - lo, 12] or None, wx, wy) matches the pairs
    lo .. hi - 1 in one call and returns an object with .matches and .counts or such a dict; ego_of(that, start [hi - lo, 12]) returns
    flow_egomotion's dict.  guess:
      "identity"   every pair in one call, without a guess, over the cold-start window spec["cold"] = (wx, wy);
      [pairs,12]   every pair in one call under the caller's motions, over (wx, wy);
      "velocity"   the pairs one after the other, each under the motion of the pair before it over (wx, wy); the first pair - under
                   spec["first"] if that is given - and every pair behind one whose fit was not ok have no guess and take the cold window.
    The fit of a pair starts from its guess.  -> {"rel": float64 [pairs,12], "ok": bool [pairs], "inliers": int64 [pairs] - the last
    round's -, "rounds": [calls], "calls": the match results, one per call, in pair order}."""
    s = flow_odometry_spec(**spec)
    rel, ok, inliers, rounds, calls = np.zeros((pairs, 12)), np.zeros(pairs, bool), np.zeros(pairs, np.int64), [], []

    def run(lo, hi, g, wx, wy):
        got = match_of(lo, hi, g, int(wx), int(wy))
        ego = ego_of(got, flow_identity(hi - lo) if g is None else g)
        rel[lo:hi], ok[lo:hi], inliers[lo:hi] = ego["poses"], ego["ok"], ego["inliers"][-1] if ego["rounds"] else 0
        rounds.append(ego["rounds"])
        calls.append(got)

    if pairs <= 0:
        pass
    elif isinstance(guess, str) and guess == "identity":
        run(0, pairs, None, *s["cold"])
    elif isinstance(guess, str) and guess == "velocity":
        last = None if s["first"] is None else np.asarray(s["first"], np.float64).reshape(1, 12)
        for k in range(pairs):
            run(k, k + 1, last, *((s["wx"], s["wy"]) if last is not None else s["cold"]))
            last = rel[k:k + 1].copy() if ok[k] else None
    elif isinstance(guess, str):
        raise ValueError("guess must be 'velocity', 'identity' or motions [%d,12], got %r" % (pairs, guess))
    else:
        g = np.asarray(guess, np.float64)
        if g.shape != (pairs, 12):
            raise ValueError("guess must be 'velocity', 'identity' or motions [%d,12], got shape %s" % (pairs, g.shape))
        run(0, pairs, np.ascontiguousarray(g), s["wx"], s["wy"])
    return {"rel": rel, "ok": ok, "inliers": inliers, "rounds": rounds, "calls": calls}


def flow_pose_lines(poses):
    """'x y yaw' per frame, the lines --poses reads, from poses float64 [B,12] (frame to world): x = t[0], y = t[1], yaw = atan2(R[1,0],
    R[0,0]); the numbers by repr, so that reading gives back the doubles."""
    p = np.asarray(poses, np.float64).reshape(-1, 12)
    return ["%r %r %r" % (float(q[9]), float(q[10]), float(np.arctan2(q[3], q[0]))) for q in p]


WARP_E_MAX = 4            # a source covers (e + 1)^2 target pixels, e <= e_max <= 4
WARP_PD_MAX = 2 ** 20     # a predicted disparity in 1/16 px that is kept: 1 .. 2^20
WARP_TOL_MAX = 2 ** 20    # tol_q at most, 1/16 px
WARP_REL_MAX = 256        # rel_q at most: t = tol_q + ((rel_q ex) >> 8)
WARP_BATCH_MAX = 65535
WARP_MODES = {"fill": 0, "confirm": 1, "reject": 2}
WARP_COUNTS = ("kept", "covered") + VOXEL_RENDER_LABELS  # the eight words of counts


def warp_words(e_max=1, tol_q=16, rel_q=0, mode="fill"):
    """The words of a disparity_warp call as a dict of ints, after the checks the C entry makes (ValueError): e_max in 0 .. 4, tol_q in
    0 .. 2^20 (1/16 px), rel_q in 0 .. 256, mode "fill", "confirm" or "reject" (or 0, 1, 2)."""
    w = {}
    for k, v, lo, hi in (("e_max", e_max, 0, WARP_E_MAX), ("tol_q", tol_q, 0, WARP_TOL_MAX), ("rel_q", rel_q, 0, WARP_REL_MAX)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (k, lo, hi, v))
        w[k] = int(v)
    if isinstance(mode, str) and mode in WARP_MODES:
        w["mode"] = WARP_MODES[mode]
    elif not isinstance(mode, (bool, str)) and isinstance(mode, (int, np.integer)) and 0 <= mode <= 2:
        w["mode"] = int(mode)
    else:
        raise ValueError("mode must be one of %s, got %r" % (sorted(WARP_MODES, key=WARP_MODES.get), mode))
    return w


def _warp_setup(d_prev, d_cur, poses):
    d_prev = np.asarray(d_prev)
    if d_prev.dtype != np.float32 or d_prev.ndim != 3:
        raise ValueError("d_prev must be float32 [B,H,W], got %s %s" % (d_prev.dtype, d_prev.shape))
    B, H, W = d_prev.shape
    if B > WARP_BATCH_MAX or not (1 <= W <= 8192 and 1 <= H <= 8192):
        raise ValueError("at most 65535 frames of at most 8192 x 8192, got %s" % (d_prev.shape,))
    if d_cur is not None:
        d_cur = np.asarray(d_cur)
        if d_cur.dtype != np.float32 or d_cur.shape != d_prev.shape:
            raise ValueError("d_cur must be float32 %s or None, got %s %s" % (d_prev.shape, d_cur.dtype, d_cur.shape))
    poses = np.asarray(poses, np.float64)
    if poses.shape != (B, 12):
        raise ValueError("poses must be float64 [%d,12], got %s" % (B, poses.shape))
    return d_prev, d_cur, poses


def _warp_compare(d_cur, ex, w):
    """label uint8 and out float32 of one frame from its d_cur float32 [H,W] and expected int64 [H,W]."""
    mq = _flow_dq(d_cur)
    t = w["tol_q"] + ((w["rel_q"] * ex) >> 8)
    label = np.where(mq == 0, np.where(ex > 0, 2, 0), np.where(ex == 0, 1, np.where(mq > ex + t, 4, np.where(mq < ex - t, 5, 3)))).astype(np.uint8)
    bits = np.ascontiguousarray(d_cur).view(np.uint32)
    none = np.uint32(0xBF800000)  # -1.0f
    if w["mode"] == 0:
        fill = (ex.astype(np.float32) / np.float32(16.0)).view(np.uint32)  # ex <= 2^20: exact
        o = np.where(mq > 0, bits, np.where(ex > 0, fill, none))
    elif w["mode"] == 1:
        o = np.where(label == 3, bits, none)
    else:
        o = np.where((label == 1) | (label == 3), bits, none)
    return label, o.astype(np.uint32).view(np.float32)


def disparity_warp(d_prev, d_cur, camera, poses, e_max=1, tol_q=16, rel_q=0, mode="fill"):
    """The disparity maps of frames k - 1 warped into frames k and compared with what frames k measured: the definition of
    include/stereo_vision_hip.h (AA) in numpy.  d_prev float32 [B,H,W]; d_cur float32 [B,H,W] or None; camera: voxel_render_camera's dict
    (flow_camera reads it); poses float64 [B,12]: previous camera to current camera, in flow_egomotion's layout.
      sources     every pixel (u0, v0) with d0q = _flow_dq(d_prev) >= 1, its index src = v0 W + u0.
      moved       X0 = _flow_point(...), Xc = _flow_move(pose, ...): doubles, one operation at a time.
      kept        z = Xc.z > FLOW_Z_MIN (false for NaN); pd = floor(16 (fb / z) + 0.5) in 1 .. 2^20; tu = floor(((f Xc.x) / z + cx) + 0.5), tv
                  = floor(((f Xc.y) / z + cy) + 0.5) with |tu|, |tv| <= 2^20 - flow_match's centre.
      footprint   e = min(e_max, (pd + d0q - 1) // d0q - 1): a point that came closer covers (tu + dx, tv + dy), dx, dy in 0 .. e, inside
                  the image.
      winner      per target pixel the largest pd, among equals the smallest src.
    -> {"expected": int32 [B,H,W], the winner's pd or 0; "source": int32 [B,H,W], the winner's src or -1; "counts": int32 [B,8] =
    WARP_COUNTS: sources kept, covers inside the image (once per source), pixels per label; "label", "out": None without a d_cur}.  With
    d_cur: mq = _flow_dq(d_cur), ex = expected, t = tol_q + ((rel_q ex) >> 8); label uint8 [B,H,W] in VOXEL_RENDER_LABELS' order: 0
    neither, 1 measured only, 2 expected only, 3 agree |mq - ex| <= t, 4 nearer mq > ex + t, 5 farther mq < ex - t; out float32 [B,H,W]: mode
    "fill" - d_cur's bits where measured, else float32(ex) / 16 where expected, else -1; "confirm" - d_cur's bits where the label is 3,
    else -1; "reject" - d_cur's bits where the label is 1 or 3, else -1.  Without d_cur the counts take the labels as 0 and 2."""
    w = warp_words(e_max, tol_q, rel_q, mode)
    cam = flow_camera(camera)
    d_prev, d_cur, poses = _warp_setup(d_prev, d_cur, poses)
    B, H, W = d_prev.shape
    expected, source, counts = np.zeros((B, H, W), np.int32), np.full((B, H, W), -1, np.int32), np.zeros((B, 8), np.int32)
    label = out = None
    if d_cur is not None:
        label, out = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.float32)
    for b in range(B):
        d0 = _flow_dq(d_prev[b]).ravel()
        src = np.flatnonzero(d0 > 0)
        q = d0[src]
        x, y, z = _flow_point(cam, src % W, src // W, q)
        X = _flow_move(poses[b], x, y, z)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            keep = X[2] > FLOW_Z_MIN  # false for NaN
            zs = np.where(keep, X[2], 1.0)
            pd = np.floor(16.0 * (cam["fb"] / zs) + 0.5)
            tu, tv = np.floor(((cam["f"] * X[0]) / zs + cam["cx"]) + 0.5), np.floor(((cam["f"] * X[1]) / zs + cam["cy"]) + 0.5)
            keep &= (pd >= 1) & (pd <= WARP_PD_MAX) & (np.abs(tu) <= FLOW_CENTRE_MAX) & (np.abs(tv) <= FLOW_CENTRE_MAX)  # false for NaN
        src, q, pd, tu, tv = src[keep], q[keep], pd[keep].astype(np.int64), tu[keep].astype(np.int64), tv[keep].astype(np.int64)
        e = np.minimum(w["e_max"], (pd + q - 1) // q - 1)
        key = (pd << 32) | (0xFFFFFFFF - src)
        keys = np.zeros(H * W, np.int64)
        covered = 0
        for dy in range(w["e_max"] + 1):
            for dx in range(w["e_max"] + 1):
                tx, ty = tu + dx, tv + dy
                hit = (e >= dx) & (e >= dy) & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                np.maximum.at(keys, ty[hit] * W + tx[hit], key[hit])
                covered += int(hit.sum())
        ex = (keys >> 32).reshape(H, W)
        expected[b] = ex
        source[b] = np.where(keys > 0, 0xFFFFFFFF - (keys & 0xFFFFFFFF), -1).reshape(H, W)
        if d_cur is not None:
            label[b], out[b] = _warp_compare(d_cur[b], ex, w)
            lab = label[b]
        else:
            lab = np.where(ex > 0, 2, 0)
        counts[b] = [len(src), covered] + [int(v) for v in np.bincount(lab.ravel(), minlength=6)]
    return {"expected": expected, "source": source, "label": label, "out": out, "counts": counts}


def disparity_warp_brute(d_prev, d_cur, camera, poses, e_max=1, tol_q=16, rel_q=0, mode="fill"):
    """disparity_warp pixel by pixel in Python floats and ints: what the tests hold the numpy form against."""
    import math
    import struct
    w = warp_words(e_max, tol_q, rel_q, mode)
    cam = flow_camera(camera)
    d_prev, d_cur, poses = _warp_setup(d_prev, d_cur, poses)
    B, H, W = d_prev.shape
    f, cx, cy, b16, fb, fb16 = (float(cam[k]) for k in ("f", "cx", "cy", "b16", "fb", "fb16"))

    def dq(d):
        d = float(d)
        if not (d > 0.0) or not math.isfinite(d):
            return 0
        v = math.floor(d * 16.0 + 0.5)
        return v if 1 <= v <= FLOW_DQ_MAX else 0

    def rounded(v):  # floor(v + 0.5) as an int, None where v is not finite
        v = v + 0.5
        return math.floor(v) if math.isfinite(v) else None

    expected, source, counts = np.zeros((B, H, W), np.int32), np.full((B, H, W), -1, np.int32), np.zeros((B, 8), np.int32)
    label = out = None
    if d_cur is not None:
        label, out = np.zeros((B, H, W), np.uint8), np.zeros((B, H, W), np.float32)
    for b in range(B):
        P = [float(v) for v in poses[b]]
        best = {}
        kept = covered = 0
        for v0 in range(H):
            for u0 in range(W):
                d0q = dq(d_prev[b, v0, u0])
                if d0q < 1:
                    continue
                d = float(d0q)
                x0, y0, z0 = ((float(u0) - cx) * b16) / d, ((float(v0) - cy) * b16) / d, fb16 / d
                x, y, z = (((P[3 * k] * x0 + P[3 * k + 1] * y0) + P[3 * k + 2] * z0) + P[9 + k] for k in range(3))
                if not z > FLOW_Z_MIN:
                    continue
                pd, tu, tv = rounded(16.0 * (fb / z)), rounded((f * x) / z + cx), rounded((f * y) / z + cy)
                if pd is None or tu is None or tv is None or not 1 <= pd <= WARP_PD_MAX or abs(tu) > 2 ** 20 or abs(tv) > 2 ** 20:
                    continue
                kept += 1
                e = min(w["e_max"], (pd + d0q - 1) // d0q - 1)
                src = v0 * W + u0
                for dy in range(e + 1):
                    for dx in range(e + 1):
                        tx, ty = tu + dx, tv + dy
                        if 0 <= tx < W and 0 <= ty < H:
                            covered += 1
                            old = best.get((ty, tx))
                            if old is None or pd > old[0] or (pd == old[0] and src < old[1]):
                                best[(ty, tx)] = (pd, src)
        hist = [0] * 6
        for v in range(H):
            for u in range(W):
                ex, src = best.get((v, u), (0, -1))
                expected[b, v, u], source[b, v, u] = ex, src
                if d_cur is None:
                    hist[2 if ex > 0 else 0] += 1
                    continue
                mq = dq(d_cur[b, v, u])
                t = w["tol_q"] + ((w["rel_q"] * ex) >> 8)
                if mq == 0:
                    lab = 2 if ex > 0 else 0
                elif ex == 0:
                    lab = 1
                else:
                    lab = 4 if mq > ex + t else 5 if mq < ex - t else 3
                hist[lab] += 1
                label[b, v, u] = lab
                own = d_cur[b, v, u:u + 1].view(np.uint32)[0]
                if w["mode"] == 0:
                    bits = own if mq > 0 else struct.unpack("<I", struct.pack("<f", ex / 16.0))[0] if ex > 0 else 0xBF800000
                elif w["mode"] == 1:
                    bits = own if lab == 3 else 0xBF800000
                else:
                    bits = own if lab in (1, 3) else 0xBF800000
                out[b, v, u:u + 1].view(np.uint32)[0] = bits
        counts[b] = [kept, covered] + hist
    return {"expected": expected, "source": source, "label": label, "out": out, "counts": counts}


TRACK_BOXES_MAX = 64         # boxes per frame: a match's membership in the boxes of one frame is one 64-bit word
TRACK_BAND_MAX = 2 ** 20     # band_q at most, 1/16 px
TRACK_GATE_MAX = 2 ** 20     # gate_m at most, 1/1024 m; 0: no gate
TRACK_SHARE_MAX = 256        # share at most: 256 votes >= share members
TRACK_M_MAX = 2 ** 20        # |m|, |ru|, |rv|, |rd| of a match are clamped to it: 1024 m, 65536 px
TRACK_P_MAX = 2 ** 30        # |p| of a match is clamped to it
TRACK_BATCH_MAX = 65535
TRACK_SUMS = ("n", "inside", "ru", "rv", "rd", "E", "mx", "my", "mz", "mxx", "myy", "mzz", "px", "py", "pz", "zero")  # the 16 words per box
TRACK_WORDS = dict(band_q=48, min_votes=3, share=128, gate_m=0)  # the defaults: 3 px about the box's disparity, half of the members


def track_words(max_boxes, width, height, band_q=48, min_votes=3, share=128, gate_m=0):
    """The words of an object_links call as a dict of ints, after the checks the C entry makes (ValueError): max_boxes in 0 .. 64, width
    and height in 1 .. 8192, band_q in 0 .. 2^20 (1/16 px), min_votes >= 1, share in 0 .. 256, gate_m in 0 .. 2^20 (1/1024 m, 0: no gate)."""
    w = {}
    for k, v, lo, hi in (("max_boxes", max_boxes, 0, TRACK_BOXES_MAX), ("width", width, 1, 8192), ("height", height, 1, 8192), ("band_q", band_q, 0, TRACK_BAND_MAX),
                         ("min_votes", min_votes, 1, 2 ** 31 - 1), ("share", share, 0, TRACK_SHARE_MAX), ("gate_m", gate_m, 0, TRACK_GATE_MAX)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (k, lo, hi, v))
        w[k] = int(v)
    return w


def _track_setup(matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1, centre):
    matches, counts, poses = _flow_sums_setup(matches, counts, poses)
    B = matches.shape[0]
    boxes0 = np.asarray(boxes0)
    if boxes0.dtype != np.int32 or boxes0.ndim != 3 or boxes0.shape[0] != B or boxes0.shape[2] != 4 or boxes0.shape[1] > TRACK_BOXES_MAX:
        raise ValueError("boxes0 must be int32 [%d,max_boxes,4] with max_boxes <= 64, got %s %s" % (B, boxes0.dtype, boxes0.shape))
    M = boxes0.shape[1]
    boxes1 = np.asarray(boxes1)
    if boxes1.dtype != np.int32 or boxes1.shape != (B, M, 4):
        raise ValueError("boxes1 must be int32 [%d,%d,4], got %s %s" % (B, M, boxes1.dtype, boxes1.shape))
    out = [matches, counts, poses, boxes0, boxes1]
    for n, what in ((n0, "n0"), (n1, "n1")):
        n = np.full(B, M, np.int32) if n is None else np.asarray(n)
        if n.dtype != np.int32 or n.shape != (B,):
            raise ValueError("%s must be None or int32 [%d], got %s %s" % (what, B, n.dtype, n.shape))
        out.append(np.clip(n.astype(np.int64), 0, M))
    for q, what in ((q0, "q0"), (q1, "q1")):
        q = np.asarray(q)
        if q.dtype != np.int32 or q.shape != (B, M):
            raise ValueError("%s must be int32 [%d,%d], got %s %s" % (what, B, M, q.dtype, q.shape))
        out.append(q.astype(np.int64))
    if centre is not None:
        centre = np.asarray(centre)
        if centre.dtype != np.int32 or centre.shape != (B, M, 3):
            raise ValueError("centre must be None or int32 [%d,%d,3], got %s %s" % (B, M, centre.dtype, centre.shape))
        centre = centre.astype(np.int64)
    return out + [centre]


def _track_link(votes, M, min_votes, share):
    """Rule 3 on the votes int [M, M + 1] of one frame, in Python integers -> link int [M, 4]."""
    link = np.zeros((M, 4), np.int64)
    link[:, 0] = -1
    keep = []
    for i in range(M):
        row = [int(v) for v in votes[i, :M]]
        members = int(votes[i, M])
        best = max(row)
        j = row.index(best)  # the lowest among equals
        second = max(row[:j] + row[j + 1:], default=0)
        link[i] = (-1, best, members, second)
        if best >= min_votes and 256 * best >= share * members:
            keep.append((j, -best, i))
    taken = set()
    for j, _, i in sorted(keep):  # per j the most votes, among equals the lowest i
        if j not in taken:
            taken.add(j)
            link[i, 0] = j
    return link


def object_links(matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1, camera, width, height, band_q=48, min_votes=3, share=128, gate_m=0, centre=None):
    """The boxes of frame k - 1 linked to those of frame k by the temporal matches that lie in both, and each linked box's matches reduced
    to the box's own motion - the definition of include/stereo_vision_hip.h (AB) in numpy.  matches int32 [B,capacity,6] and counts int32
    [B]: flow_match's, under flow_pose_sums' rules (a count of -1 or 0 gives nothing, a count above the capacity counts as the capacity, a
    row with d0q outside 1 .. 2^20 is skipped); poses float64 [B,12]: previous camera to current camera; boxes0 int32 [B,M,4] = (x, y, w, h),
    n0 int32 [B] or None (M each; clamped to 0 .. M) and q0 int32 [B,M]: the boxes of frame k - 1 with a reference disparity each in
    quarter pixels - objects' info[..., 3], box_positions' stat[..., 2]; q <= 0: no depth test -; boxes1, n1, q1: the same of frame k; M
    <= 64; camera: voxel_render_camera's dict; band_q in 1/16 px, min_votes >= 1, share in 0 .. 256, gate_m in 1/1024 m (0: no gate),
    centre int32 [B,M,3] or None.
      members   a box's pixels are box_bounds': columns [clamp(x), clamp(x + w)), rows [clamp(y), clamp(y + h)).  in0(i): (u0, v0) in box i of
                frame k - 1, and q0[i] <= 0 or |d0q - 4 q0[i]| <= band_q.  in1(j): (u1, v1) in box j of frame k, and q1[j] <= 0 or (d1q > 0
                and |d1q - 4 q1[j]| <= band_q).
      votes     int32 [B,M,M+1]: votes[i][j] = the matches with in0(i) and in1(j); votes[i][M] = the matches with in0(i).
      link      j*(i) = the j with the most votes, among equals the lowest; kept if votes[i][j*] >= min_votes and 256 votes[i][j*] >= share
                members; of several i that keep one j only that with the most votes keeps it, among equals the lowest i.  int32 [B,M,4]
                = (j or -1, votes[i][j*], members, the most votes over j != j*).
      sums      int64 [B,M,16], TRACK_SUMS, per linked box i over the matches with in0(i), in1(link[i]) and d1q in 1 .. 2^20: Xc = the
                match's point moved by the pose (_flow_point, _flow_move), X1 = _flow_point of (u1, v1, d1q); inside: Xc.z > FLOW_Z_MIN and
                flow_pose_sums' |pu|, |pv|, |pd| <= 2^30.  m_a = clamp(floor(1024 (X1_a - Xc_a) + 0.5), +-2^20), p_a = clamp(floor(1024 X1_a +
                0.5), +-2^30), ru, rv, rd flow_pose_sums' residuals clamped to +-2^20.  With a centre and gate_m > 0 a match counts only if
                |m_a - centre[i][a]| <= gate_m on the three axes.  (n, inside, sum ru, rv, rd, sum ru^2 + rv^2, sum m[3], sum m^2[3], sum p[3],
                0): inside is counted in front of the gate, everything else behind it.
    Rows at and behind n0 and columns at and behind n1 are 0, their link (-1, 0, 0, 0).  -> {"votes", "link", "sums"}."""
    matches, counts, poses, boxes0, boxes1, n0, n1, q0, q1, centre = _track_setup(matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1, centre)
    B, cap = matches.shape[:2]
    M = boxes0.shape[1]
    w = track_words(M, width, height, band_q, min_votes, share, gate_m)
    cam = flow_camera(camera)
    votes, link, sums = np.zeros((B, M, M + 1), np.int32), np.zeros((B, M, 4), np.int32), np.zeros((B, M, 16), np.int64)
    link[:, :, 0] = -1
    gated = centre is not None and w["gate_m"] > 0

    def members(u, v, d, boxes, n, q, needs_d):
        bounds = np.array([box_bounds(bx, width, height) for bx in boxes], np.int64).reshape(M, 4)
        ok = (u[:, None] >= bounds[:, 0]) & (u[:, None] < bounds[:, 1]) & (v[:, None] >= bounds[:, 2]) & (v[:, None] < bounds[:, 3]) & (np.arange(M) < n)
        near = np.abs(d[:, None] - 4 * q) <= w["band_q"]
        if needs_d:
            near &= d[:, None] > 0
        return ok & ((q <= 0) | near)

    for b in range(B):
        n = min(int(counts[b]), cap)
        if n <= 0 or M == 0:
            continue
        m = matches[b, :n].astype(np.int64)
        u0, v0, d0, u1, v1, d1 = (m[:, k] for k in range(6))
        live = (d0 >= 1) & (d0 <= FLOW_DQ_MAX)
        in0 = members(u0, v0, d0, boxes0[b], n0[b], q0[b], False) & live[:, None]
        in1 = members(u1, v1, d1, boxes1[b], n1[b], q1[b], True)
        votes[b, :, :M] = in0.T.astype(np.int64) @ in1.astype(np.int64)
        votes[b, :, M] = in0.sum(0)
        link[b] = _track_link(votes[b], M, w["min_votes"], w["share"])
        if not (link[b, :, 0] >= 0).any():
            continue
        both = live & (d1 >= 1) & (d1 <= FLOW_DQ_MAX)
        x0, y0, z0 = _flow_point(cam, u0, v0, np.where(live, d0, 1))
        x, y, z = _flow_move(poses[b], x0, y0, z0)
        X1 = _flow_point(cam, u1, v1, np.where(both, d1, 1))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ok = both & (z > FLOW_Z_MIN)
            zs = np.where(ok, z, 1.0)
            xz, yz, bz = x / zs, y / zs, cam["fb"] / zs
            pu, pv, pd = np.floor(16.0 * (cam["f"] * xz + cam["cx"]) + 0.5), np.floor(16.0 * (cam["f"] * yz + cam["cy"]) + 0.5), np.floor(16.0 * bz + 0.5)
            inside = ok & (np.abs(pu) <= FLOW_PIXEL_MAX) & (np.abs(pv) <= FLOW_PIXEL_MAX) & (np.abs(pd) <= FLOW_PIXEL_MAX)
            mv = [np.where(inside, _flow_q(1024.0 * (np.where(inside, X1[a] - c, 0.0)), TRACK_M_MAX), 0) for a, c in enumerate((x, y, z))]
            pq = [np.where(inside, _flow_q(1024.0 * X1[a], TRACK_P_MAX), 0) for a in range(3)]
        pu, pv, pd = (np.where(inside, p, 0.0).astype(np.int64) for p in (pu, pv, pd))
        r = [np.where(inside, np.clip(v, -TRACK_M_MAX, TRACK_M_MAX), 0) for v in (16 * u1 - pu, 16 * v1 - pv, d1 - pd)]
        for i in np.flatnonzero(link[b, :, 0] >= 0):
            fed = in0[:, i] & in1[:, link[b, i, 0]] & both
            ins = fed & inside
            cnt = ins
            if gated:
                cnt = ins & np.logical_and.reduce([np.abs(mv[a] - centre[b, i, a]) <= w["gate_m"] for a in range(3)])
            s = [cnt.sum(), ins.sum(), r[0][cnt].sum(), r[1][cnt].sum(), r[2][cnt].sum(), (r[0][cnt] ** 2 + r[1][cnt] ** 2).sum()]
            s += [mv[a][cnt].sum() for a in range(3)] + [(mv[a][cnt] ** 2).sum() for a in range(3)] + [pq[a][cnt].sum() for a in range(3)] + [0]
            sums[b, i] = s
    return {"votes": votes, "link": link, "sums": sums}


def object_links_brute(matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1, camera, width, height, band_q=48, min_votes=3, share=128, gate_m=0, centre=None):
    """object_links match by match: Python floats in the stated order in front of the rounding, Python integers behind it."""
    import math
    matches, counts, poses, boxes0, boxes1, n0, n1, q0, q1, centre = _track_setup(matches, counts, poses, boxes0, n0, q0, boxes1, n1, q1, centre)
    B, cap = matches.shape[:2]
    M = boxes0.shape[1]
    w = track_words(M, width, height, band_q, min_votes, share, gate_m)
    cam = flow_camera(camera)
    f, cx, cy, b16, fb, fb16 = (cam[k] for k in ("f", "cx", "cy", "b16", "fb", "fb16"))
    votes, link, sums = np.zeros((B, M, M + 1), np.int32), np.zeros((B, M, 4), np.int32), np.zeros((B, M, 16), np.int64)
    link[:, :, 0] = -1

    def rnd(v, lim):  # clamp(floor(v + 0.5), +-lim) of a double that is not NaN
        t = v + 0.5
        return lim if t >= lim else -lim if t <= -lim else math.floor(t)

    def inside_box(u, v, box):
        i_lb, i_ub, j_lb, j_ub = box_bounds(box, width, height)
        return i_lb <= u < i_ub and j_lb <= v < j_ub

    for b in range(B):
        rows = [[int(v) for v in matches[b, i]] for i in range(max(min(int(counts[b]), cap), 0))]
        rows = [r for r in rows if 1 <= r[2] <= FLOW_DQ_MAX]
        mem = []
        for u0, v0, d0, u1, v1, d1 in rows:
            a0 = [i for i in range(int(n0[b])) if inside_box(u0, v0, boxes0[b, i]) and (q0[b, i] <= 0 or abs(d0 - 4 * int(q0[b, i])) <= w["band_q"])]
            a1 = [j for j in range(int(n1[b])) if inside_box(u1, v1, boxes1[b, j]) and (q1[b, j] <= 0 or (d1 > 0 and abs(d1 - 4 * int(q1[b, j])) <= w["band_q"]))]
            mem.append((a0, a1))
            for i in a0:
                votes[b, i, M] += 1
                for j in a1:
                    votes[b, i, j] += 1
        link[b] = _track_link(votes[b], M, w["min_votes"], w["share"])
        p = [float(v) for v in poses[b]]
        for (u0, v0, d0, u1, v1, d1), (a0, a1) in zip(rows, mem):
            feeds = [i for i in a0 if link[b, i, 0] in a1]
            if not feeds or not 1 <= d1 <= FLOW_DQ_MAX:
                continue
            X0 = (((u0 - cx) * b16) / d0, ((v0 - cy) * b16) / d0, fb16 / d0)
            X1 = (((u1 - cx) * b16) / d1, ((v1 - cy) * b16) / d1, fb16 / d1)
            Xc = [((p[3 * k] * X0[0] + p[3 * k + 1] * X0[1]) + p[3 * k + 2] * X0[2]) + p[9 + k] for k in range(3)]
            z = Xc[2]
            if not z > FLOW_Z_MIN:
                continue
            xz, yz, bz = Xc[0] / z, Xc[1] / z, fb / z
            pred = (16.0 * (f * xz + cx) + 0.5, 16.0 * (f * yz + cy) + 0.5, 16.0 * bz + 0.5)
            if not all(math.isfinite(v) and abs(math.floor(v)) <= FLOW_PIXEL_MAX for v in pred):
                continue
            pu, pv, pd = (math.floor(v) for v in pred)
            res = [max(-TRACK_M_MAX, min(TRACK_M_MAX, v)) for v in (16 * u1 - pu, 16 * v1 - pv, d1 - pd)]
            mv = [rnd(1024.0 * (X1[a] - Xc[a]), TRACK_M_MAX) for a in range(3)]
            pq = [rnd(1024.0 * X1[a], TRACK_P_MAX) for a in range(3)]
            for i in feeds:
                s = [int(v) for v in sums[b, i]]
                s[1] += 1
                if centre is None or w["gate_m"] == 0 or all(abs(mv[a] - int(centre[b, i, a])) <= w["gate_m"] for a in range(3)):
                    add = [1, 0, res[0], res[1], res[2], res[0] ** 2 + res[1] ** 2] + mv + [v * v for v in mv] + pq + [0]
                    s = [x + y for x, y in zip(s, add)]
                sums[b, i] = s
    return {"votes": votes, "link": link, "sums": sums}


def object_centre(sums):
    """The centre of a gated round from the sums of a round: floor(sum m / n + 1/2) per axis in Python integers, int32 [...,3]; 0 where n = 0."""
    s = np.asarray(sums, np.int64)
    out = np.zeros(s.shape[:-1] + (3,), np.int32)
    for at in np.ndindex(*s.shape[:-1]):
        n = int(s[at][0])
        if n > 0:
            out[at] = [(2 * int(s[at][6 + a]) + n) // (2 * n) for a in range(3)]
    return out


def object_motion(sums, link=None, dt=1.0):
    """What the sums of object_links say per box of frame k - 1, in the current camera's axes: {"motion": float64 [...,3] = sum m / n / 1024 /
    dt - metres per frame for dt = 1, metres per second for the frames' distance in seconds; the object's own motion, because Xc already
    carries the camera's -, "position": float64 [...,3] = sum p / n / 1024, the mean of the box's points in frame k, "n": int64 [...]}.  NaN
    where n = 0, or where `link` is given and says -1."""
    s = np.asarray(sums, np.int64)
    n = s[..., 0].copy()
    if link is not None:
        n = np.where(np.asarray(link)[..., 0] >= 0, n, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.where(n > 0, n, 1).astype(np.float64)[..., None]
        motion = np.where(n[..., None] > 0, s[..., 6:9].astype(np.float64) / den / 1024.0 / float(dt), np.nan)
        position = np.where(n[..., None] > 0, s[..., 12:15].astype(np.float64) / den / 1024.0, np.nan)
    return {"motion": motion, "position": position, "n": n}


def object_links_rounds(links_of, gate_m):
    """flow_egomotion's idiom for a gate: a round without one, then - for gate_m > 0 - a round gated about the first round's mean.
    links_of(gate_m, centre) -> object_links' dict, from the numpy definition or from the device; -> the last round's dict, with
    "centre" int32 [B,M,3] (None for gate_m = 0)."""
    got = dict(links_of(0, None))
    got["centre"] = None
    if gate_m > 0:
        centre = object_centre(np.asarray(got["sums"].cpu().numpy() if hasattr(got["sums"], "cpu") else got["sums"]))
        got = dict(links_of(int(gate_m), centre))
        got["centre"] = centre
    return got


class ObjectTracks:
    """Host bookkeeping over object_links' results, in plain Python - the role of the reference's tracker: a track keeps its id along
    links, an unlinked current box opens a new id (in ascending j), a track without a link ends.  Per track the last `history` motions
    (those with n >= min_n), their mean, the velocity = mean / dt in m/s, moving = |velocity| > move_m, and predicted = pos + mean: the
    constant-velocity prediction of where the box is a frame later, in the current camera's axes."""

    def __init__(self, history=5, min_n=8, move_m=1.0, dt=0.1):
        if int(history) < 1 or not float(dt) > 0:
            raise ValueError("history must be >= 1 and dt > 0, got %r and %r" % (history, dt))
        self.history, self.min_n, self.move_m, self.dt = int(history), int(min_n), float(move_m), float(dt)
        self.frame, self.next_id, self.tracks = -1, 0, []  # tracks: one per box of the last frame, in box order

    def _open(self, box, pos):
        t = {"id": self.next_id, "box": tuple(int(v) for v in box), "pos": tuple(float(v) for v in pos), "motions": [], "n": 0}
        self.next_id += 1
        return self._derive(t)

    def _derive(self, t):
        if t["motions"]:
            mean = tuple(sum(m[a] for m in t["motions"]) / len(t["motions"]) for a in range(3))
        else:
            mean = (float("nan"),) * 3
        t["mean"] = mean
        t["velocity"] = tuple(v / self.dt for v in mean)
        speed = sum(v * v for v in t["velocity"]) ** 0.5
        t["moving"] = bool(speed > self.move_m)  # False for NaN
        t["predicted"] = tuple(p + (0.0 if v != v else v) for p, v in zip(t["pos"], mean))
        return t

    def start(self, boxes, positions):
        """The first frame: every box opens a track.  boxes [n,4], positions [n,3] -> the tracks."""
        self.frame, self.tracks = self.frame + 1, [self._open(bx, ps) for bx, ps in zip(boxes, positions)]
        return self.tracks

    def step(self, link, motion, n, boxes, positions):
        """One pair: link [n_prev] = the current box of each box of the last frame or -1 (object_links' link[..., 0]), motion [n_prev,3] in
        metres per frame and n [n_prev] (object_motion's), boxes [n_cur,4] and positions [n_cur,3] of the current frame -> its tracks."""
        if self.frame < 0:
            raise ValueError("step() before start()")
        if len(link) < len(self.tracks):
            raise ValueError("link has %d rows for %d tracks" % (len(link), len(self.tracks)))
        new = [None] * len(boxes)
        for i, old in enumerate(self.tracks):
            j = int(link[i])
            if j < 0 or j >= len(boxes) or new[j] is not None:
                continue  # the track ends
            mv = tuple(float(v) for v in motion[i])
            motions = list(old["motions"])
            if int(n[i]) >= self.min_n and all(v == v for v in mv):
                motions = (motions + [mv])[-self.history:]
            new[j] = self._derive({"id": old["id"], "box": tuple(int(v) for v in boxes[j]), "pos": tuple(float(v) for v in positions[j]), "motions": motions,
                                   "n": int(n[i])})
        for j in range(len(boxes)):
            if new[j] is None:
                new[j] = self._open(boxes[j], positions[j])
        self.frame, self.tracks = self.frame + 1, new
        return self.tracks

    def feed(self, tracked):
        """A batch as StereoRig.track returns it (numpy): {"boxes" [F,M,4], "n" [F], "positions" [F,M,3], "link" [F-1,M,4], "motion" [F-1,M,3],
        "count" [F-1,M]}.  The first frame of a batch that is not the first one fed is the last frame of the batch before it and is not
        counted again.  -> per frame that was new, (frame, a copy of its tracks)."""
        out = []
        boxes, n, pos = np.asarray(tracked["boxes"]), np.asarray(tracked["n"]), np.asarray(tracked["positions"])
        if self.frame < 0 and len(boxes):
            out.append((0, [dict(t) for t in self.start(boxes[0][:n[0]], pos[0][:n[0]])]))
        for k in range(1, len(boxes)):
            link = np.asarray(tracked["link"])[k - 1][:n[k - 1], 0]
            tr = self.step(link, np.asarray(tracked["motion"])[k - 1], np.asarray(tracked["count"])[k - 1], boxes[k][:n[k]], pos[k][:n[k]])
            out.append((self.frame, [dict(t) for t in tr]))
        return out

    def lines(self, frame, tracks):
        """'frame id x y w h X Y Z vx vy vz n moving' per track: what --tracks writes; floats by repr."""
        return ["%d %d %d %d %d %d %r %r %r %r %r %r %d %d" % ((frame, t["id"]) + t["box"] + t["pos"] + t["velocity"] + (t["n"], int(t["moving"]))) for t in tracks]


PLACE_RINGS_MAX = 64         # rings of a descriptor at most: a ring key is 64 bytes
PLACE_SECTORS_MIN, PLACE_SECTORS_MAX = 8, 128  # sectors: a multiple of 4 - four bytes per v_sad_u8 -, two shifts per lane at most
PLACE_BINS_MAX = 4096        # rings * sectors at most: 255 * 4096 < 2^20, so (sad << 8) | shift fits 32 bits
PLACE_Q = 1024               # a row's x and y in units of r_max / 1024
PLACE_DIR = 2 ** 14          # the length of a sector's direction
PLACE_QUERIES_MAX = 65535
PLACE_KEYS_MAX = 2 ** 20
PLACE_BATCH_MAX = 65535
PLACE_ACCEPT_MAX = 2 ** 20   # accept at most: 256 sad <= accept norm, 256 = every candidate (sad <= norm)
PLACE_WORDS = ("sum", "occupied", "kept", "dropped")  # the four words of a descriptor
PLACE_NONE = (-1, 0, -1, 0)  # best of a query without a candidate


def _place_int(v, lo, hi, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    return int(v)


def place_params(r_max, rings=20, sectors=60, z_lo=-0.5, z_hi=4.5, r_min=0.0):
    """The words of place recognition (sv_place_spec) as a dict, after the checks the C entry makes (ValueError): r_max finite > 0, z_lo <
    z_hi finite, 0 <= r_min < r_max, rings in 1 .. 64, sectors a multiple of 4 in 8 .. 128, rings * sectors <= 4096.  With them unit =
    r_max / 1024 and z_unit = (z_hi - z_lo) / 255 in double, ring_edge2 int64 [rings + 1] = (1024 r // rings)^2, r_min2 = floor(r_min /
    unit)^2, and dirs int32 [sectors,2] = (rint(2^14 cos(2 pi k / S)), rint(2^14 sin(2 pi k / S))): the table the device takes as it is."""
    R, S = _place_int(rings, 1, PLACE_RINGS_MAX, "rings"), _place_int(sectors, PLACE_SECTORS_MIN, PLACE_SECTORS_MAX, "sectors")
    if S % 4 or R * S > PLACE_BINS_MAX:
        raise ValueError("sectors must be a multiple of 4 and rings * sectors <= 4096, got %d and %d" % (R, S))
    r_max, z_lo, z_hi, r_min = (float(v) for v in (r_max, z_lo, z_hi, r_min))
    if not (np.isfinite([r_max, z_lo, z_hi, r_min]).all() and r_max > 0 and z_lo < z_hi and 0 <= r_min < r_max):
        raise ValueError("place_params needs finite words with r_max > 0, z_lo < z_hi and 0 <= r_min < r_max, got %r" % ((r_max, z_lo, z_hi, r_min),))
    unit, z_unit = np.float64(r_max) / 1024.0, (np.float64(z_hi) - np.float64(z_lo)) / 255.0
    if not (unit > 0 and np.isfinite(z_unit) and z_unit > 0):
        raise ValueError("r_max / 1024 and (z_hi - z_lo) / 255 must be finite and > 0")
    ang = 2.0 * np.pi * np.arange(S, dtype=np.float64) / S
    dirs = np.stack([np.rint(PLACE_DIR * np.cos(ang)), np.rint(PLACE_DIR * np.sin(ang))], -1).astype(np.int32)
    return {"r_max": r_max, "rings": R, "sectors": S, "z_lo": z_lo, "z_hi": z_hi, "r_min": r_min, "unit": float(unit), "z_unit": float(z_unit),
            "ring_edge2": (PLACE_Q * np.arange(R + 1, dtype=np.int64) // R) ** 2, "r_min2": int(np.floor(np.float64(r_min) / unit)) ** 2, "dirs": dirs}


def _place_setup(xyz, n, counts, params, poses):
    """The checked arguments of place_descriptor, and per row of [B,cap]: is it one of the frame's, x, y, z in double (in the vehicle's
    axes: under the pose where there is one), its weight."""
    w = place_params(params["r_max"], params["rings"], params["sectors"], params["z_lo"], params["z_hi"], params["r_min"])
    xyz = np.asarray(xyz)
    if xyz.dtype not in (np.float32, np.float64) or xyz.ndim != 3 or xyz.shape[2] != 3 or xyz.shape[0] > PLACE_BATCH_MAX:
        raise ValueError("xyz must be float32 or float64 [B,cap,3] with B <= 65535, got %s %s" % (xyz.dtype, xyz.shape))
    B, cap = xyz.shape[:2]
    counts = np.asarray(counts)
    if counts.shape != (B,) or counts.dtype.kind != "i":
        raise ValueError("counts must be an integer array [%d], got %s %s" % (B, counts.dtype, counts.shape))
    if n is not None and (np.asarray(n).shape != (B, cap) or np.asarray(n).dtype.kind != "i"):
        raise ValueError("n must be an integer array [B,cap] or None")
    rows = np.arange(cap)[None, :] < np.minimum(counts.astype(np.int64), cap)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):  # rows beyond counts may hold anything
        if poses is None:
            P = xyz.astype(np.float64)
        else:
            poses = np.asarray(poses, np.float64)
            if poses.shape != (B, 12):
                raise ValueError("poses must be None or [%d,12], got %s" % (B, poses.shape))
            P = _voxel_map_world(xyz, poses)
    wt = np.ones((B, cap), np.int64) if n is None else np.asarray(n).astype(np.int64)
    return w, B, cap, rows, P, wt


def _place_outputs(B, R, S):
    return {"desc": np.zeros((B, R, S), np.uint8), "ring": np.zeros((B, R), np.uint8), "words": np.zeros((B, 4), np.int32)}


def _place_finish(out):
    """ring and words[:, :2] from desc."""
    out["ring"][:] = (out["desc"] > 0).sum(2)  # at most 128
    out["words"][:, 0] = out["desc"].astype(np.int64).sum((1, 2))
    out["words"][:, 1] = (out["desc"] > 0).sum((1, 2))
    return out


def place_descriptor(xyz, n, counts, params, poses=None):
    """The polar height descriptors of B frames of rows, the definition of include/stereo_vision_hip.h (AC1) in numpy.  xyz float32 or
    float64 [B,cap,3] in the vehicle's axes (x forward, y left, z up), n int [B,cap] or None (every weight 1), counts int [B] - frame b has
    its first min(counts[b], cap) rows, none for counts[b] <= 0 -, params: place_params' dict; poses float64 [B,12] or None: applied first,
    by voxel_map_insert's transform.  A row is kept iff n >= 1, x, y, z are finite, |x| < r_max and |y| < r_max and z_lo <= z < z_hi in
    double, and with qx = int(floor(x / unit)), qy likewise, d2 = qx^2 + qy^2: r_min2 <= d2 < 1024^2 and (qx, qy) != (0, 0).  Its ring is
    the largest r with ring_edge2[r] <= d2, its sector the one k with cross(dir[k], q) >= 0 and cross(dir[k + 1 mod S], q) < 0 (all S are
    evaluated and exactly one must hold), its code 1 + min(254, int(floor((z - z_lo) / z_unit))).
    -> {"desc" uint8 [B,R,S]: per bin the largest code, 0 for an empty bin; "ring" uint8 [B,R]: the occupied sectors per ring; "words"
    int32 [B,4] = (the sum of the codes, the occupied bins, the kept rows, the dropped rows)}."""
    w, B, cap, rows, P, wt = _place_setup(xyz, n, counts, params, poses)
    R, S, dirs = w["rings"], w["sectors"], w["dirs"].astype(np.int64)
    out = _place_outputs(B, R, S)
    x, y, z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        keep = rows & (wt >= 1) & np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        keep &= (np.abs(x) < w["r_max"]) & (np.abs(y) < w["r_max"]) & (w["z_lo"] <= z) & (z < w["z_hi"])
    b_of = np.broadcast_to(np.arange(B)[:, None], (B, cap))[keep]
    qx, qy = np.floor(x[keep] / np.float64(w["unit"])).astype(np.int64), np.floor(y[keep] / np.float64(w["unit"])).astype(np.int64)
    d2 = qx * qx + qy * qy
    ok = (w["r_min2"] <= d2) & (d2 < PLACE_Q * PLACE_Q) & ((qx != 0) | (qy != 0))
    b_of, qx, qy, d2, zk = b_of[ok], qx[ok], qy[ok], d2[ok], z[keep][ok]
    ring = np.searchsorted(w["ring_edge2"], d2, side="right") - 1
    cross = dirs[None, :, 0] * qy[:, None] - dirs[None, :, 1] * qx[:, None]  # [N,S]
    hit = (cross >= 0) & (np.roll(cross, -1, axis=1) < 0)
    assert (hit.sum(1) == 1).all(), "a row lies in no sector or in two"
    sector = hit.argmax(1)
    code = 1 + np.minimum(254, np.floor((zk - np.float64(w["z_lo"])) / np.float64(w["z_unit"])).astype(np.int64))
    np.maximum.at(out["desc"], (b_of, ring, sector), code.astype(np.uint8))
    out["words"][:, 2] = np.bincount(b_of, minlength=B)
    out["words"][:, 3] = rows.sum(1) - out["words"][:, 2]
    return _place_finish(out)


def place_descriptor_brute(xyz, n, counts, params, poses=None):
    """place_descriptor row by row, in Python numbers."""
    w, B, cap, rows, P, wt = _place_setup(xyz, n, counts, params, poses)
    R, S = w["rings"], w["sectors"]
    dirs, edge2 = [(int(a), int(b)) for a, b in w["dirs"]], [int(e) for e in w["ring_edge2"]]
    unit, z_unit, z_lo = np.float64(w["unit"]), np.float64(w["z_unit"]), np.float64(w["z_lo"])
    out = _place_outputs(B, R, S)
    for b in range(B):
        for i in range(cap):
            if not rows[b, i]:
                continue
            x, y, z = P[b, i]
            good = wt[b, i] >= 1 and np.isfinite(x) and np.isfinite(y) and np.isfinite(z) and abs(x) < w["r_max"] and abs(y) < w["r_max"] and w["z_lo"] <= z < w["z_hi"]
            if good:
                qx, qy = int(np.floor(x / unit)), int(np.floor(y / unit))
                d2 = qx * qx + qy * qy
                good = w["r_min2"] <= d2 < PLACE_Q * PLACE_Q and (qx, qy) != (0, 0)
            if not good:
                out["words"][b, 3] += 1
                continue
            ring = max(r for r in range(R) if edge2[r] <= d2)
            cr = [d[0] * qy - d[1] * qx for d in dirs]
            ks = [k for k in range(S) if cr[k] >= 0 and cr[(k + 1) % S] < 0]
            assert len(ks) == 1, "a row lies in no sector or in two"
            code = 1 + min(254, int(np.floor((z - z_lo) / z_unit)))
            out["desc"][b, ring, ks[0]] = max(int(out["desc"][b, ring, ks[0]]), code)
            out["words"][b, 2] += 1
    return _place_finish(out)


def _place_match_setup(q_desc, q_words, q_ring, q_seq, k_desc, k_words, k_ring, k_seq, min_gap, ring_gate, max_shift, accept):
    q_desc, k_desc = np.asarray(q_desc), np.asarray(k_desc)
    if q_desc.dtype != np.uint8 or q_desc.ndim != 3 or k_desc.dtype != np.uint8 or k_desc.ndim != 3 or q_desc.shape[1:] != k_desc.shape[1:]:
        raise ValueError("q_desc and k_desc must be uint8 [Q,R,S] and [K,R,S], got %s %s and %s %s" % (q_desc.dtype, q_desc.shape, k_desc.dtype, k_desc.shape))
    (Q, R, S), K = q_desc.shape, k_desc.shape[0]
    _place_int(R, 1, PLACE_RINGS_MAX, "rings"), _place_int(S, PLACE_SECTORS_MIN, PLACE_SECTORS_MAX, "sectors")
    if S % 4 or R * S > PLACE_BINS_MAX or Q > PLACE_QUERIES_MAX or K > PLACE_KEYS_MAX:
        raise ValueError("place_match needs sectors a multiple of 4, rings * sectors <= 4096, Q <= 65535 and K <= 2^20")
    arrays = []
    for a, what, shape, dtype in ((q_words, "q_words", (Q, 4), np.int32), (q_ring, "q_ring", (Q, R), np.uint8), (q_seq, "q_seq", (Q,), np.int32),
                                  (k_words, "k_words", (K, 4), np.int32), (k_ring, "k_ring", (K, R), np.uint8), (k_seq, "k_seq", (K,), np.int32)):
        a = np.asarray(a)
        if a.dtype != dtype or a.shape != shape:
            raise ValueError("%s must be %s %s, got %s %s" % (what, np.dtype(dtype).name, list(shape), a.dtype, a.shape))
        arrays.append(a.astype(np.int64))
    min_gap, ring_gate = _place_int(min_gap, 0, 2 ** 31 - 1, "min_gap"), _place_int(ring_gate, -1, 2 ** 31 - 1, "ring_gate")
    max_shift = S if max_shift is None else _place_int(max_shift, 0, PLACE_SECTORS_MAX, "max_shift")
    accept = _place_int(accept, 0, PLACE_ACCEPT_MAX, "accept")
    shifts = [s for s in range(S) if min(s, S - s) <= max_shift]
    return [q_desc.astype(np.int64), k_desc.astype(np.int64)] + arrays + [Q, K, R, S, min_gap, ring_gate, shifts, accept]


def _place_better(sad_a, norm_a, sad_b, norm_b):
    """sad_a / norm_a < sad_b / norm_b by the cross-multiplied compare, in Python integers."""
    return int(sad_a) * int(norm_b) < int(sad_b) * int(norm_a)


def _place_pick(Q, K, evaluated, accept, want_pair):
    """The outputs of place_match from evaluated(q) -> (before the gate, [(key, sad, shift, norm), ...] in key order)."""
    best, counts = np.zeros((Q, 4), np.int32), np.zeros((Q, 3), np.int32)
    pair = np.zeros((Q, K, 2), np.int32) if want_pair else None
    if want_pair:
        pair[:, :, 0] = -1
    for q in range(Q):
        before, cands = evaluated(q)
        top = None
        for k, sad, s, norm in cands:
            if want_pair:
                pair[q, k] = (sad, s)
            if top is None or _place_better(sad, norm, top[1], top[3]):  # ties keep the lower key
                top = (k, sad, s, norm)
        ok = top is not None and 256 * top[1] <= accept * top[3]
        best[q] = PLACE_NONE if top is None else (top[0] if ok else -1, top[2], top[1], top[3])
        counts[q] = (before, len(cands), int(ok))
    out = {"best": best, "counts": counts}
    if want_pair:
        out["pair"] = pair
    return out


def place_match(q_desc, q_words, q_ring, q_seq, k_desc, k_words, k_ring, k_seq, min_gap, ring_gate=-1, max_shift=None, accept=256, want_pair=False):
    """Q query descriptors against K stored ones under every rotation, the definition of include/stereo_vision_hip.h (AC2) in numpy.
    q_desc uint8 [Q,R,S], q_words int32 [Q,4], q_ring uint8 [Q,R] (place_descriptor's), q_seq int32 [Q]: the queries' sequence numbers;
    k_* the same of the K keys.  Key k is a candidate of query q iff both sums (words[0]) are > 0 and |q_seq - k_seq| >= min_gap - counted
    in counts[q, 0] -, and, unless ring_gate < 0, sum_r |q_ring[r] - k_ring[r]| <= ring_gate - counts[q, 1].  For a candidate sad(s) = sum
    |q[r,c] - k[r,(c + s) mod S]| over s in 0 .. S - 1 with min(s, S - s) <= max_shift (None: every s); its result is the least sad, among
    equals the least s; norm = q_sum + k_sum.  The best key has the least sad / norm by sad_a norm_b < sad_b norm_a, among equals the
    least index; it is accepted iff 256 sad <= accept norm.
    -> {"best" int32 [Q,4] = (key or -1, shift, sad, norm; (-1, 0, -1, 0) without a candidate), "counts" int32 [Q,3] = (before the gate,
    behind it, accepted ? 1 : 0), and with want_pair "pair" int32 [Q,K,2] = (sad or -1, shift; (-1, 0) where not evaluated)}."""
    qd, kd, qw, qr, qs, kw, kr, ks, Q, K, R, S, min_gap, ring_gate, shifts, accept = _place_match_setup(
        q_desc, q_words, q_ring, q_seq, k_desc, k_words, k_ring, k_seq, min_gap, ring_gate, max_shift, accept)

    def evaluated(q):
        pre = (kw[:, 0] > 0) & (qw[q, 0] > 0) & (np.abs(qs[q] - ks) >= min_gap)
        post = pre if ring_gate < 0 else pre & (np.abs(qr[q][None] - kr).sum(1) <= ring_gate)
        idx = np.flatnonzero(post)
        if not len(idx):
            return int(pre.sum()), []
        sad = np.stack([np.abs(qd[q][None] - np.roll(kd[idx], -s, axis=2)).sum((1, 2)) for s in shifts], 1)  # [C, shifts]
        at = sad.argmin(1)  # the first of the least: the least s
        return int(pre.sum()), [(int(k), int(sad[i, at[i]]), shifts[at[i]], int(qw[q, 0] + kw[k, 0])) for i, k in enumerate(idx)]

    return _place_pick(Q, K, evaluated, accept, want_pair)


def place_match_brute(q_desc, q_words, q_ring, q_seq, k_desc, k_words, k_ring, k_seq, min_gap, ring_gate=-1, max_shift=None, accept=256, want_pair=False):
    """place_match pair by pair and shift by shift."""
    qd, kd, qw, qr, qs, kw, kr, ks, Q, K, R, S, min_gap, ring_gate, shifts, accept = _place_match_setup(
        q_desc, q_words, q_ring, q_seq, k_desc, k_words, k_ring, k_seq, min_gap, ring_gate, max_shift, accept)
    cols = np.arange(S)

    def evaluated(q):
        before, cands = 0, []
        for k in range(K):
            if not (qw[q, 0] > 0 and kw[k, 0] > 0 and abs(int(qs[q]) - int(ks[k])) >= min_gap):
                continue
            before += 1
            if ring_gate >= 0 and sum(abs(int(a) - int(b)) for a, b in zip(qr[q], kr[k])) > ring_gate:
                continue
            top = None
            for s in shifts:
                sad = int(np.abs(qd[q] - kd[k][:, (cols + s) % S]).sum())
                if top is None or sad < top[0]:
                    top = (sad, s)
            cands.append((k, top[0], top[1], int(qw[q, 0]) + int(kw[k, 0])))
        return before, cands

    return _place_pick(Q, K, evaluated, accept, want_pair)


def place_yaw(shift, sectors):
    """The heading of the query in the key's frame, in radians, for place_match's shift: 2 pi shift / sectors wrapped to (-pi, pi]."""
    s = np.asarray(shift, np.int64) % int(sectors)
    return np.pi * (2.0 * np.where(2 * s > sectors, s - sectors, s) / float(sectors))  # the quotient first: half a turn is pi itself


def place_guess(key_pose, shift, sectors):
    """float64 [..., 4] = (x, y, z, yaw), the guess VoxelMap.localize takes: the key's position - key_pose [..., 12], voxel_map_pose's
    layout - with its heading, atan2(R[1,0], R[0,0]), turned by place_yaw(shift, sectors) and wrapped to (-pi, pi]."""
    p = np.asarray(key_pose, np.float64)
    yaw = np.arctan2(p[..., 3], p[..., 0]) + place_yaw(shift, sectors)
    yaw = np.pi - np.mod(np.pi - yaw, 2.0 * np.pi)  # (-pi, pi]
    return np.stack([p[..., 9], p[..., 10], p[..., 11], yaw], -1)


def place_lines(frames, best, sectors):
    """'frame key shift sad norm yaw_deg' per accepted query: what --places writes; the angle by repr."""
    return ["%d %d %d %d %d %r" % (f, b[0], b[1], b[2], b[3], float(np.degrees(place_yaw(b[1], sectors)))) for f, b in zip(frames, np.asarray(best)) if b[0] >= 0]


GROUND_BINS_MIN, GROUND_BINS_MAX = 8, 4096
GROUND_VH_MIN, GROUND_TOL_MAX, GROUND_G_TOL_MAX, GROUND_HEIGHT_MAX = -32768, 16, 4096, 32768
GROUND_LABELS = {"invalid": 0, "ground": 1, "obstacle": 2, "below": 3}


def ground_params(height, disp_max=None, n_bins=None, vh_lo=0, vh_hi=None, vh_step=2, qb_step=2, tol=2, g_tol=4, min_run=8, min_support=0):
    """The nine words of sv_ground_spec as a dict of ints, after the checks sv_ground_disparity_device makes (ValueError for a bad
    argument).  n_bins = 4 (disp_max + 1) unless given: 8 <= n_bins <= 4096; vh_hi None = height - 2;
    -32768 <= vh_lo <= vh_hi <= height - 2; vh_step >= 1; 1 <= qb_step < n_bins (so that a candidate exists); 0 <= tol <= 16;
    0 <= g_tol <= 4096; min_run >= 1; min_support >= 0; 1 <= height <= 32768."""
    if n_bins is None:
        if disp_max is None:
            raise ValueError("give disp_max or n_bins")
        n_bins = 4 * (int(disp_max) + 1)
    if vh_hi is None:
        vh_hi = int(height) - 2
    p = dict(n_bins=n_bins, vh_lo=vh_lo, vh_hi=vh_hi, vh_step=vh_step, qb_step=qb_step, tol=tol, g_tol=g_tol, min_run=min_run, min_support=min_support)
    for k, v in p.items():
        if isinstance(v, (bool, np.bool_)) or int(v) != v or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("%s must be an int32, got %r" % (k, v))
        p[k] = int(v)
    if isinstance(height, bool) or int(height) != height or not 1 <= height <= GROUND_HEIGHT_MAX:
        raise ValueError("height must be an integer in 1 .. %d, got %r" % (GROUND_HEIGHT_MAX, height))
    if not GROUND_BINS_MIN <= p["n_bins"] <= GROUND_BINS_MAX:
        raise ValueError("n_bins = %d outside %d .. %d" % (p["n_bins"], GROUND_BINS_MIN, GROUND_BINS_MAX))
    if not GROUND_VH_MIN <= p["vh_lo"] <= p["vh_hi"] <= int(height) - 2:
        raise ValueError("the horizon rows need %d <= vh_lo <= vh_hi <= height - 2, got %d .. %d at height %d" % (GROUND_VH_MIN, p["vh_lo"], p["vh_hi"], height))
    if p["vh_step"] < 1 or not 1 <= p["qb_step"] < p["n_bins"]:
        raise ValueError("vh_step must be >= 1 and qb_step in 1 .. n_bins - 1, got %d and %d" % (p["vh_step"], p["qb_step"]))
    if not 0 <= p["tol"] <= GROUND_TOL_MAX or not 0 <= p["g_tol"] <= GROUND_G_TOL_MAX:
        raise ValueError("tol must be in 0 .. %d and g_tol in 0 .. %d, got %d and %d" % (GROUND_TOL_MAX, GROUND_G_TOL_MAX, p["tol"], p["g_tol"]))
    if p["min_run"] < 1 or p["min_support"] < 0:
        raise ValueError("min_run must be >= 1 and min_support >= 0, got %d and %d" % (p["min_run"], p["min_support"]))
    return p


def ground_quantise(disp, n_bins):
    """(q int32, valid bool) per pixel of a float32 map: valid = d > 0 (NaN is not), q = min(round_half_even(4 d), n_bins - 1) where
    valid, 0 elsewhere - quarter-pixel bins, the box median's quantisation with n_bins in place of 4096."""
    d = np.asarray(disp, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = d > 0
        q = np.where(valid, np.minimum(np.rint(d * np.float32(4.0)), np.float32(n_bins - 1)), np.float32(0)).astype(np.int32)
    return q, valid


def v_disparity(disp, n_bins):
    """The v-disparity histogram uint32 [H, n_bins] of a float32 map [H,W] ([B,H,n_bins] of [B,H,W]): per row the number of valid
    pixels in each bin of ground_quantise."""
    q, valid = ground_quantise(disp, n_bins)
    if q.ndim not in (2, 3):
        raise ValueError("expected disp [H,W] or [B,H,W], got shape %s" % (q.shape,))
    rows = q.reshape(-1, q.shape[-1])
    ok = valid.reshape(rows.shape)
    out = np.zeros((rows.shape[0], n_bins), np.uint32)
    for v in range(rows.shape[0]):
        out[v] = np.bincount(rows[v][ok[v]], minlength=n_bins)
    return out.reshape(q.shape[:-1] + (n_bins,))


def ground_row_bins(vh, qb, height):
    """g(v) int64 [height]: the ground line's bin per row - ql(v) = (2 qb (v - vh) + den) // (2 den), den = height - 1 - vh, below the
    horizon row (v > vh), 0 at and above it.  ql(height - 1) = qb."""
    v = np.arange(height, dtype=np.int64)
    den = height - 1 - int(vh)
    return np.where(v > vh, (2 * int(qb) * (v - int(vh)) + den) // (2 * den), 0)


def ground_line(vdisp, vh_lo, vh_hi, vh_step, qb_step, tol, min_support=0):
    """The ground line of one v-disparity histogram [H, n_bins]: (vh, qb, S, n_valid) as Python ints, by exhaustive search over the
    horizon rows vh = vh_lo, vh_lo + vh_step, ... <= vh_hi and the bottom-row bins qb = qb_step, 2 qb_step, ... < n_bins.
    S(vh, qb) = the histogram's mass within tol bins of ql(v) on the rows max(vh + 1, 0) .. H - 1 (bins outside 0 .. n_bins - 1 hold
    nothing).  The largest S wins, ties go to the smallest vh, then the smallest qb; S < min_support gives (-1, -1, S, n_valid)."""
    h = np.asarray(vdisp).astype(np.int64)
    H, n_bins = h.shape
    ground_params(H, n_bins=n_bins, vh_lo=vh_lo, vh_hi=vh_hi, vh_step=vh_step, qb_step=qb_step, tol=tol, min_support=min_support)
    P = np.zeros((H, n_bins + 1), np.int64)
    P[:, 1:] = np.cumsum(h, axis=1)
    qbs = np.arange(qb_step, n_bins, qb_step, dtype=np.int64)
    best = None
    for vh in range(vh_lo, vh_hi + 1, vh_step):
        den = H - 1 - vh
        v = np.arange(max(vh + 1, 0), H, dtype=np.int64)[:, None]
        ql = (2 * qbs[None, :] * (v - vh) + den) // (2 * den)
        S = (P[v, np.minimum(ql + tol + 1, n_bins)] - P[v, np.maximum(ql - tol, 0)]).sum(0)
        i = int(np.argmax(S))  # the first of equal maxima: the smallest qb
        if best is None or S[i] > best[2]:  # strictly: the smallest vh stays
            best = (vh, int(qbs[i]), int(S[i]))
    n_valid = int(h.sum())
    return (best[0], best[1], best[2], n_valid) if best[2] >= min_support else (-1, -1, best[2], n_valid)


def ground_labels(disp, n_bins, vh, qb, g_tol):
    """Labels uint8 [H,W] of a float32 map against the ground line (vh, qb): with e = q - g(v) (ground_quantise, ground_row_bins)
    0 invalid, 1 ground (|e| <= g_tol), 2 obstacle (e > g_tol: nearer than the ground), 3 below the ground (e < -g_tol).
    (vh, qb) = (-1, -1), "no ground": every valid pixel is 3."""
    q, valid = ground_quantise(disp, n_bins)
    if q.ndim != 2:
        raise ValueError("expected disp [H,W], got shape %s" % (q.shape,))
    if qb < 0:
        return np.where(valid, 3, 0).astype(np.uint8)
    e = q.astype(np.int64) - ground_row_bins(vh, qb, q.shape[0])[:, None]
    return np.where(valid, np.where(e > g_tol, 2, np.where(e < -g_tol, 3, 1)), 0).astype(np.uint8)


def free_space(labels, disp, min_run):
    """(free_row int32 [W], free_disp float32 [W]): per column, walking up from the bottom row, the first row v whose min_run rows
    v, v - 1, ..., v - min_run + 1 all exist and are labelled obstacle - the base of the nearest obstacle, the far end of the drivable
    stretch - and disp[v, u] there; (-1, 0) for a column without one.  An explicit walk, one column after the other."""
    lab = np.asarray(labels)
    d = np.asarray(disp, dtype=np.float32)
    H, W = lab.shape
    free_row, free_disp = np.full(W, -1, np.int32), np.zeros(W, np.float32)
    for u in range(W):
        run = 0
        for v in range(H - 1, -1, -1):
            run = run + 1 if lab[v, u] == 2 else 0
            if run == min_run:
                free_row[u], free_disp[u] = v + min_run - 1, d[v + min_run - 1, u]
                break
    return free_row, free_disp


def ground(disp, disp_max=None, **spec):
    """All of include/stereo_vision_hip.h (G) for one float32 map [H,W] in numpy: a dict with vdisp, ground (int32 [4] = vh, qb, S,
    n_valid), labels, free_row and free_disp; spec as ground_params, min_support None = the width."""
    d = np.asarray(disp, dtype=np.float32)
    if d.ndim != 2:
        raise ValueError("expected disp [H,W], got shape %s" % (d.shape,))
    if spec.get("min_support") is None:
        spec["min_support"] = d.shape[1]
    p = ground_params(d.shape[0], disp_max, **spec)
    vdisp = v_disparity(d, p["n_bins"])
    rec = ground_line(vdisp, p["vh_lo"], p["vh_hi"], p["vh_step"], p["qb_step"], p["tol"], p["min_support"])
    labels = ground_labels(d, p["n_bins"], rec[0], rec[1], p["g_tol"])
    free_row, free_disp = free_space(labels, d, p["min_run"])
    return {"vdisp": vdisp, "ground": np.array(rec, np.int32), "labels": labels, "free_row": free_row, "free_disp": free_disp}


def ground_pose(Q, vh, qb, height):
    """(height_m, pitch_rad, slope_px_per_row) of the camera over the ground line (vh, qb) of maps with `height` rows, in float64:
    with f = Q[2][3], cy = -Q[1][3] and the baseline 1 / |Q[3][2]|, the line d(v) = slope (v - vh), slope = qb / (4 den) pixels of
    disparity per row (den = height - 1 - vh), is a plane at height = baseline cos(pitch) / slope under a camera pitched by
    pitch = atan((cy - vh) / f) (positive: looking down).  ValueError for "no ground" (qb < 1)."""
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    den = int(height) - 1 - int(vh)
    if qb < 1 or den < 1:
        raise ValueError("no ground line: vh = %r, qb = %r at height %r" % (vh, qb, height))
    f, cy, baseline = Q[2, 3], -Q[1, 3], 1.0 / abs(Q[3, 2])
    slope = float(qb) / (4.0 * den)
    pitch = float(np.arctan((cy - float(vh)) / f))
    return float(baseline * np.cos(pitch) / slope), pitch, slope


def free_space_points(Q, free_row, free_disp, XR=None, XT=None):
    """float64 [W,3] ([B,W,3] for [B,W] input): the 3-D point of each column's obstacle base - reproject()'s arithmetic in its "d1"
    form on pixel (u, free_row[u]) with disparity free_disp[u], then XR P + XT -, NaN where free_row < 0."""
    row, d = np.asarray(free_row), np.asarray(free_disp, dtype=np.float32).astype(np.float64)
    if row.shape != d.shape or row.ndim not in (1, 2):
        raise ValueError("free_row and free_disp must both be [W] or [B,W], got %s / %s" % (row.shape, d.shape))
    Q = np.asarray(Q, np.float64).reshape(4, 4)
    x, y = np.broadcast_to(np.arange(row.shape[-1], dtype=np.float64), row.shape), row.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pos = [((Q[r, 0] * x + Q[r, 1] * y) + Q[r, 2] * d) + Q[r, 3] for r in range(4)]
        X, Y, Z = pos[0] / pos[3], pos[1] / pos[3], pos[2] / pos[3]
        if XR is not None or XT is not None:
            XR = np.eye(3) if XR is None else np.asarray(XR, np.float64).reshape(3, 3)
            XT = np.zeros(3) if XT is None else np.asarray(XT, np.float64).reshape(3)
            X, Y, Z = [((XR[r, 0] * X + XR[r, 1] * Y) + XR[r, 2] * Z) + XT[r] for r in range(3)]
    P = np.stack([X, Y, Z], -1)
    P[row < 0] = np.nan
    return P


STIXEL_Q_MIN_MAX, STIXEL_SIM_MAX, STIXEL_GAP_MAX, STIXEL_LAYERS_MAX = 4095, 4096, 255, 64
_STIXEL_WORDS = ("q_min", "sim", "max_gap", "min_rows", "max_layers", "col_step", "sim_cols", "min_cols")


def stixel_params(disp_max=None, n_bins=None, q_min=16, sim=6, max_gap=2, min_rows=8, max_layers=8, col_step=1, sim_cols=8, min_cols=16):
    """The nine words of sv_stixel_spec as a dict of ints, after the checks sv_stixel_disparity_device makes (ValueError for a bad
    argument).  n_bins = 4 (disp_max + 1) unless given: 8 <= n_bins <= 4096; 0 <= q_min <= 4095; 0 <= sim <= 4096; 0 <= max_gap <= 255;
    min_rows >= 1; 1 <= max_layers <= 64; col_step >= 1; 0 <= sim_cols <= 4096; min_cols >= 1."""
    if n_bins is None:
        if disp_max is None:
            raise ValueError("give disp_max or n_bins")
        n_bins = 4 * (int(disp_max) + 1)
    p = dict(n_bins=n_bins, q_min=q_min, sim=sim, max_gap=max_gap, min_rows=min_rows, max_layers=max_layers, col_step=col_step, sim_cols=sim_cols,
             min_cols=min_cols)
    for k, v in p.items():
        if isinstance(v, (bool, np.bool_)) or int(v) != v or not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("%s must be an int32, got %r" % (k, v))
        p[k] = int(v)
    if not GROUND_BINS_MIN <= p["n_bins"] <= GROUND_BINS_MAX:
        raise ValueError("n_bins = %d outside %d .. %d" % (p["n_bins"], GROUND_BINS_MIN, GROUND_BINS_MAX))
    if not 0 <= p["q_min"] <= STIXEL_Q_MIN_MAX:
        raise ValueError("q_min must be in 0 .. %d, got %d" % (STIXEL_Q_MIN_MAX, p["q_min"]))
    if not 0 <= p["sim"] <= STIXEL_SIM_MAX or not 0 <= p["sim_cols"] <= STIXEL_SIM_MAX:
        raise ValueError("sim and sim_cols must be in 0 .. %d, got %d and %d" % (STIXEL_SIM_MAX, p["sim"], p["sim_cols"]))
    if not 0 <= p["max_gap"] <= STIXEL_GAP_MAX:
        raise ValueError("max_gap must be in 0 .. %d, got %d" % (STIXEL_GAP_MAX, p["max_gap"]))
    if not 1 <= p["max_layers"] <= STIXEL_LAYERS_MAX:
        raise ValueError("max_layers must be in 1 .. %d, got %d" % (STIXEL_LAYERS_MAX, p["max_layers"]))
    if p["min_rows"] < 1 or p["col_step"] < 1 or p["min_cols"] < 1:
        raise ValueError("min_rows, col_step and min_cols must be >= 1, got %d, %d and %d" % (p["min_rows"], p["col_step"], p["min_cols"]))
    return p


def stixels(disp, labels, disp_max=None, **spec):
    """(stixels int32 [max_layers, Wv, 4], n_stixels int32 [Wv]) of one float32 map [H,W] and its labels uint8 [H,W]
    (ground_labels'), Wv = ceil(W / col_step): the definition of include/stereo_vision_hip.h (H) as an explicit walk, one visited
    column (u % col_step == 0) after the other.  A pixel is foreground iff its label is 2, d > 0 and q = ground_quantise's bin
    >= q_min.  From row H - 1 upwards: a foreground row v starts a run with base qb = q[v]; a row above matches iff it is foreground
    and |q - qb| <= sim (against the base, not the neighbour); the run ends at the top or after max_gap + 1 consecutive rows that
    do not match; t = its last matching row, n = its matching rows.  n >= min_rows makes it a stixel (v, t, qb, n); the walk goes
    on at row t - 1 either way.  The first max_layers stixels of a column, bottom-up, are stored, -1 beyond the column's count;
    n_stixels is not capped.  spec as stixel_params (sim_cols and min_cols are not used here)."""
    p = stixel_params(disp_max, **spec)
    d, lab = np.asarray(disp, dtype=np.float32), np.asarray(labels)
    if d.ndim != 2 or lab.shape != d.shape:
        raise ValueError("expected disp [H,W] and labels of the same shape, got %s / %s" % (d.shape, lab.shape))
    q, valid = ground_quantise(d, p["n_bins"])
    q = np.where((lab == 2) & valid & (q >= p["q_min"]), q, -1)  # -1: not foreground
    H, W = d.shape
    cols = range(0, W, p["col_step"])
    out, count = np.full((p["max_layers"], len(cols), 4), -1, np.int32), np.zeros(len(cols), np.int32)
    for i, u in enumerate(cols):
        c = q[:, u].tolist()
        v = H - 1
        while v >= 0:
            if c[v] < 0:
                v -= 1
                continue
            qb, t, n, gap, r = c[v], v, 1, 0, v - 1
            while r >= 0 and gap <= p["max_gap"]:
                if c[r] >= 0 and abs(c[r] - qb) <= p["sim"]:
                    t, n, gap = r, n + 1, 0
                else:
                    gap += 1
                r -= 1
            if n >= p["min_rows"]:
                if count[i] < p["max_layers"]:
                    out[count[i], i] = (v, t, qb, n)
                count[i] += 1
            v = t - 1
    return out, count


def stixel_objects(layer0, col_step=1, sim_cols=8, min_cols=16, capacity=None):
    """(boxes int32 [n,4], info int32 [n,4], count) from the first layer of stixels() ([Wv,4]): an object is a maximal run of
    consecutive visited columns that each have a stixel and whose q_base differs from the previous visited column's by at most
    sim_cols, kept iff it spans >= min_cols visited columns; left to right.  boxes = (x, y, w, h) = (first column, smallest v_top,
    last column - first column + 1, largest v_bottom - y + 1) in pixels - the box layout of box_positions -, info = (n_cols, q_lo,
    q_hi, q_med) with q_med the lower median of the columns' q_base (the smallest value whose cumulative count reaches
    (n_cols + 1) // 2).  count is not capped; n = min(count, capacity) rows are returned (capacity None = all)."""
    p = stixel_params(n_bins=GROUND_BINS_MIN, col_step=col_step, sim_cols=sim_cols, min_cols=min_cols)
    if capacity is not None and (isinstance(capacity, bool) or int(capacity) != capacity or not 0 <= capacity < 2 ** 31):
        raise ValueError("capacity must be an integer >= 0, got %r" % (capacity,))
    s = np.asarray(layer0)
    if s.ndim != 2 or s.shape[1] != 4:
        raise ValueError("expected the first layer of stixels [Wv,4], got shape %s" % (s.shape,))
    boxes, info = [], []
    i, n = 0, s.shape[0]
    while i < n:
        if s[i, 0] < 0:
            i += 1
            continue
        j = i
        while j + 1 < n and s[j + 1, 0] >= 0 and abs(int(s[j + 1, 2]) - int(s[j, 2])) <= p["sim_cols"]:
            j += 1
        if j - i + 1 >= p["min_cols"]:
            seg = s[i:j + 1].astype(np.int64)
            y = int(seg[:, 1].min())
            qs = np.sort(seg[:, 2])
            boxes.append((i * p["col_step"], y, (j - i) * p["col_step"] + 1, int(seg[:, 0].max()) - y + 1))
            info.append((j - i + 1, int(qs[0]), int(qs[-1]), int(qs[(len(qs) + 1) // 2 - 1])))
        i = j + 1
    count = len(boxes)
    keep = count if capacity is None else min(count, int(capacity))
    return np.array(boxes[:keep], np.int32).reshape(keep, 4), np.array(info[:keep], np.int32).reshape(keep, 4), count


def stixel_world(disp, disp_max=None, capacity=None, **spec):
    """ground() first, then stixels() on its labels and stixel_objects() on their first layer, for one float32 map [H,W]: ground()'s
    dict plus stixels, n_stixels, boxes, info and count.  spec: the words of ground_params and of stixel_params (n_bins is shared)."""
    d = np.asarray(disp, dtype=np.float32)
    mine = {k: spec.pop(k) for k in _STIXEL_WORDS if k in spec}
    out = ground(d, disp_max, **spec)
    mine["n_bins"] = out["vdisp"].shape[1]
    out["stixels"], out["n_stixels"] = stixels(d, out["labels"], **mine)
    p = stixel_params(**mine)
    out["boxes"], out["info"], out["count"] = stixel_objects(out["stixels"][0], p["col_step"], p["sim_cols"], p["min_cols"], capacity)
    return out


OCCUPANCY_Z_SCALE_MAX, OCCUPANCY_H_MAX, OCCUPANCY_CELL_MAX = 65536, 65535, 2 ** 24
OCCUPANCY_STATES = {"unknown": 0, "free": 1, "occupied": 2}
OCCUPANCY_PNG = np.array([0, 127, 255], np.uint8)  # --occupancy: the grey of each state
_OCCUPANCY_FULL_WALK = 1 << 16  # rays of more steps than this are walked over their clipped k range only


def occupancy_params(x_range, y_range, z_range, scale, z_scale=20, min_obstacle=3, min_ground=1, min_rays=1, XT=None):
    """(rows, cols, dict of the four integer words of sv_occupancy_spec) after the checks sv_occupancy_disparity_device makes (ValueError
    for a bad argument): top_view_grid's in "count" mode; z_scale an integer in 1 .. 65536 (height steps per metre); the three thresholds
    integers in 1 .. 2^31 - 1; with XT, the origin of the sight lines, |XT[0] scale| and |XT[1] scale| below 2^24 (NaN refused)."""
    rows, cols = top_view_grid(x_range, y_range, z_range, scale, "count")
    p = dict(z_scale=z_scale, min_obstacle=min_obstacle, min_ground=min_ground, min_rays=min_rays)
    for k, v in p.items():
        if isinstance(v, (bool, np.bool_)) or int(v) != v or not 1 <= v <= (OCCUPANCY_Z_SCALE_MAX if k == "z_scale" else 2 ** 31 - 1):
            raise ValueError("%s must be an integer in 1 .. %s, got %r" % (k, "65536" if k == "z_scale" else "2^31 - 1", v))
        p[k] = int(v)
    if XT is not None:
        o = np.asarray(XT, np.float64).reshape(3)
        with np.errstate(over="ignore", invalid="ignore"):
            if not (np.abs(o[:2] * float(int(scale))) < OCCUPANCY_CELL_MAX).all():
                raise ValueError("the origin of the sight lines, XT = %r, lies 2^24 cells or more from the frame's origin" % (o.tolist(),))
    return rows, cols, p


def occupancy_ray_clip(r0, c0, r1, c1, rows, cols, obstacle_end):
    """(k_lo, k_hi), inclusive, of the steps of the sight line from cell (r0, c0) to cell (r1, c1) whose cells lie inside a grid of
    rows x cols - (0, -1) for none - without walking it.  With dr = r1 - r0, dc = c1 - c0 and n = max(|dr|, |dc|) step k is at
    (r0 + (2 k dr + n) // (2 n), c0 + (2 k dc + n) // (2 n)); k runs over 0 .. n - 1 for an obstacle end and 0 .. n for a ground end
    (n = 0: the origin's cell alone, for a ground end).  Each coordinate is monotone in k, so per axis the admissible k form an interval:
    0 <= a0 + (2 k da + n) // (2 n) <= size - 1  <=>  n (2 lo - 1) <= 2 k da <= n (2 hi + 1) - 1  with lo = -a0, hi = size - 1 - a0.
    A line whose span misses the grid on an axis is dropped first, which also keeps every product below 2^63 in the kernel."""
    r0, c0, r1, c1 = int(r0), int(c0), int(r1), int(c1)
    dr, dc = r1 - r0, c1 - c0
    n = max(abs(dr), abs(dc))
    k_lo, k_hi = 0, (n - 1 if obstacle_end else n)
    if max(r0, r1) < 0 or min(r0, r1) > rows - 1 or max(c0, c1) < 0 or min(c0, c1) > cols - 1:
        return 0, -1
    if n == 0:
        return k_lo, k_hi  # the origin's cell, inside the grid by the test above
    for a0, da, size in ((r0, dr, rows), (c0, dc, cols)):
        lo, hi = n * (2 * (-a0) - 1), n * (2 * (size - 1 - a0) + 1) - 1
        if da == 0:
            if not lo <= 0 <= hi:
                return 0, -1
        elif da > 0:
            k_lo, k_hi = max(k_lo, -(-lo // (2 * da))), min(k_hi, hi // (2 * da))  # ceil and floor: // is the floor for either sign
        else:
            k_lo, k_hi = max(k_lo, -(-hi // (2 * da))), min(k_hi, lo // (2 * da))
    return (k_lo, k_hi) if k_lo <= k_hi else (0, -1)


def occupancy_ray_cells(r0, c0, r1, c1, obstacle_end, k_lo=0, k_hi=None):
    """(r int64 [m], c int64 [m]): the cells of the steps k_lo .. k_hi (None: the last step) of the sight line of occupancy_ray_clip,
    inside the grid or not."""
    r0, c0 = int(r0), int(c0)
    dr, dc = int(r1) - r0, int(c1) - c0
    n = max(abs(dr), abs(dc))
    last = n - 1 if obstacle_end else n
    k = np.arange(k_lo, (last if k_hi is None else k_hi) + 1, dtype=np.int64)
    if n == 0:
        return np.full(k.size, r0, np.int64), np.full(k.size, c0, np.int64)
    return r0 + (2 * k * dr + n) // (2 * n), c0 + (2 * k * dc + n) // (2 * n)


def occupancy_grid(disp, labels, free_row, free_disp, Q, x_range, y_range, z_range, scale, z_scale=20, XR=None, XT=None, min_obstacle=3,
                   min_ground=1, min_rays=1):
    """Occupancy and elevation grid of one float32 map [H,W], its labels uint8 [H,W] and its free space (free_row int32 [W], free_disp
    float32 [W]; ground()'s outputs), the definition of include/stereo_vision_hip.h (J) in numpy: a dict with
      cells  int32 [rows, cols, 4] = (n_ground, n_obstacle, h_lo, h_hi) - the pixels with d > 0 and label 1 / label 2 whose point
             (reproject()'s "d1" form, then XR P + XT) lies strictly inside the three ranges, in the cell
             (trunc(x1 s) - trunc(X s), trunc(y1 s) - trunc(Y s)) of top_view_grid(mode="count"), and the smallest and largest
             h = min(trunc((Z - z0) * z_scale), 65535) over both kinds; h_lo = h_hi = -1 for a cell without one;
      n_rays int32 [rows, cols] - the sight lines that crossed the cell: per image column one line from the cell of the camera centre
             (XT, or 0; not range-tested) to the cell of the column's obstacle base (free_row >= 0: free_space_points' point; the end cell
             itself is left out) or else of its topmost ground pixel (label 1, d > 0; the end cell is counted), by the closed form of
             occupancy_ray_clip; a column with neither, or with an end that is not finite or 2^24 cells or more from the frame's origin,
             casts none; z_range does not apply;
      state  uint8 [rows, cols] - 2 occupied iff n_obstacle >= min_obstacle, else 1 free iff n_ground >= min_ground or
             n_rays >= min_rays, else 0 unknown.
    Labels 0 and 3 never count: a map without ground (every valid pixel 3) gives an all-unknown grid."""
    rows, cols, p = occupancy_params(x_range, y_range, z_range, scale, z_scale, min_obstacle, min_ground, min_rays, XT)
    d = np.asarray(disp, dtype=np.float32)
    lab = np.asarray(labels)
    row, fd = np.asarray(free_row), np.asarray(free_disp, dtype=np.float32)
    if d.ndim != 2 or lab.shape != d.shape or row.shape != (d.shape[1],) or fd.shape != row.shape:
        raise ValueError("expected disp [H,W], labels [H,W], free_row [W] and free_disp [W], got %s / %s / %s / %s" % (d.shape, lab.shape, row.shape, fd.shape))
    H, W = d.shape
    s = float(int(scale))
    x0, x1, y0, y1, z0, z1 = (float(v) for v in (x_range[0], x_range[1], y_range[0], y_range[1], z_range[0], z_range[1]))
    R1, C1 = int(np.trunc(x1 * s)), int(np.trunc(y1 * s))
    with np.errstate(invalid="ignore"):
        valid = d > 0
    # evidence
    P = _box_points(d.astype(np.float64), Q, XR, XT)
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(invalid="ignore"):
        keep = valid & ((lab == 1) | (lab == 2)) & (X > x0) & (X < x1) & (Y > y0) & (Y < y1) & (Z > z0) & (Z < z1)
    Xk, Yk, Zk, kind = X[keep], Y[keep], Z[keep], lab[keep]
    flat = (R1 - np.trunc(Xk * s).astype(np.int64)) * cols + (C1 - np.trunc(Yk * s).astype(np.int64))
    assert flat.size == 0 or (flat.min() >= 0 and flat.max() < rows * cols)
    with np.errstate(over="ignore"):
        h = np.minimum(np.trunc((Zk - z0) * float(p["z_scale"])), float(OCCUPANCY_H_MAX)).astype(np.int64)
    cells = np.zeros((rows * cols, 4), np.int64)
    cells[:, 0] = np.bincount(flat[kind == 1], minlength=rows * cols)
    cells[:, 1] = np.bincount(flat[kind == 2], minlength=rows * cols)
    cells[:, 2], cells[:, 3] = 2 ** 31 - 1, -1
    np.minimum.at(cells[:, 2], flat, h)
    np.maximum.at(cells[:, 3], flat, h)
    cells[cells[:, 3] < 0, 2] = -1
    # sight lines
    n_rays = np.zeros(rows * cols, np.int64)
    o = np.zeros(3) if XT is None else np.asarray(XT, np.float64).reshape(3)
    r0, c0 = R1 - int(np.trunc(o[0] * s)), C1 - int(np.trunc(o[1] * s))
    ground_px = (lab == 1) & valid
    top = np.where(ground_px.any(0), ground_px.argmax(0), -1)  # the topmost ground pixel of each column
    obstacle = row >= 0
    v_end = np.where(obstacle, row, top).astype(np.int64)
    d_end = np.where(obstacle, fd, d[np.maximum(top, 0), np.arange(W)]).astype(np.float32)
    E = free_space_points(Q, v_end, d_end, XR, XT)  # NaN where v_end < 0: no ray
    with np.errstate(over="ignore", invalid="ignore"):
        tX, tY = np.trunc(E[:, 0] * s), np.trunc(E[:, 1] * s)
        cast = np.isfinite(E).all(1) & (np.abs(tX) < OCCUPANCY_CELL_MAX) & (np.abs(tY) < OCCUPANCY_CELL_MAX)
    for u in np.nonzero(cast)[0]:
        r1, c1 = R1 - int(tX[u]), C1 - int(tY[u])
        if max(abs(r1 - r0), abs(c1 - c0)) <= _OCCUPANCY_FULL_WALK:
            r, c = occupancy_ray_cells(r0, c0, r1, c1, bool(obstacle[u]))
            inside = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
            r, c = r[inside], c[inside]
        else:
            r, c = occupancy_ray_cells(r0, c0, r1, c1, bool(obstacle[u]), *occupancy_ray_clip(r0, c0, r1, c1, rows, cols, bool(obstacle[u])))
        n_rays[r * cols + c] += 1  # a line visits a cell once: its major coordinate advances with every step
    state = np.where(cells[:, 1] >= p["min_obstacle"], 2, np.where((cells[:, 0] >= p["min_ground"]) | (n_rays >= p["min_rays"]), 1, 0))
    return {"cells": cells.astype(np.int32).reshape(rows, cols, 4), "n_rays": n_rays.astype(np.int32).reshape(rows, cols),
            "state": state.astype(np.uint8).reshape(rows, cols)}


def occupancy_heights(cells, z0, z_scale):
    """(z_lo, z_hi) float64, the shape of cells[..., 0]: the heights h_lo / h_hi of occupancy_grid's cells back in metres,
    z0 + h / z_scale - the lower edge of the height step: a point with that h lies in [z, z + 1 / z_scale), and h = 65535 is open
    above - and NaN for an empty cell."""
    c = np.asarray(cells)
    if c.shape[-1] != 4:
        raise ValueError("cells must be [..., 4], got shape %s" % (c.shape,))
    if isinstance(z_scale, bool) or int(z_scale) != z_scale or not 1 <= z_scale <= OCCUPANCY_Z_SCALE_MAX:
        raise ValueError("z_scale must be an integer in 1 .. 65536, got %r" % (z_scale,))
    out = []
    for k in (2, 3):
        hk = c[..., k].astype(np.float64)
        out.append(np.where(c[..., k] >= 0, float(z0) + hk / float(int(z_scale)), np.nan))
    return out[0], out[1]


OCCUPANCY_MAP_WORDS = ("top", "left", "rows", "cols", "scale", "l_occ", "l_free", "l_min", "l_max")  # sv_occupancy_map_spec, in its order
OCCUPANCY_MAP_LOG_ODDS = {"l_occ": 85, "l_free": 40, "l_min": -200, "l_max": 350}  # log-odds times 100
OCCUPANCY_BATCH_MAX = 65535
OCCUPANCY_POSES_MAX = 65535  # candidates per frame of occupancy_match


def occupancy_map_words(map):
    """The nine words of a map - a dict or an object with these attributes (engine.SvOccupancyMapSpec) - as a dict of ints after the
    checks sv_occupancy_fuse_device makes (ValueError for a bad word): rows and cols in 1 .. 32768, scale >= 1, |top| and |left| below
    2^24, l_occ and l_free in 1 .. 32767, -32767 <= l_min <= 0 <= l_max <= 32767 and l_min < l_max."""
    w = {}
    for k in OCCUPANCY_MAP_WORDS:
        v = map[k] if isinstance(map, dict) else getattr(map, k)
        if isinstance(v, (bool, np.bool_)) or int(v) != v:
            raise ValueError("%s of the map must be an integer, got %r" % (k, v))
        w[k] = int(v)
    if not (1 <= w["rows"] <= 32768 and 1 <= w["cols"] <= 32768):
        raise ValueError("a map of %d x %d cells: 1 .. 32768 in either dimension" % (w["rows"], w["cols"]))
    if w["scale"] < 1 or w["scale"] > 2 ** 31 - 1:
        raise ValueError("the map's scale must be a positive integer, got %r" % (w["scale"],))
    if abs(w["top"]) >= OCCUPANCY_CELL_MAX or abs(w["left"]) >= OCCUPANCY_CELL_MAX:
        raise ValueError("|top| and |left| of the map must stay below 2^24, got %d, %d" % (w["top"], w["left"]))
    if not (1 <= w["l_occ"] <= 32767 and 1 <= w["l_free"] <= 32767):
        raise ValueError("l_occ and l_free must lie in 1 .. 32767, got %d, %d" % (w["l_occ"], w["l_free"]))
    if not (-32767 <= w["l_min"] <= 0 <= w["l_max"] <= 32767) or w["l_min"] == w["l_max"]:
        raise ValueError("the clamp needs -32767 <= l_min <= 0 <= l_max <= 32767 and l_min < l_max, got %d, %d" % (w["l_min"], w["l_max"]))
    return w


def occupancy_map_params(x_range, y_range, scale, l_occ=85, l_free=40, l_min=-200, l_max=350):
    """The words of the world map over x_range x y_range (integer-valued bounds, lo < hi: top_view_grid's rule) at `scale` uniform cells
    per metre: top = x1 scale, left = y1 scale, rows = (x1 - x0) scale, cols = (y1 - y0) scale, and the four log-odds words (times 100),
    checked as occupancy_map_words does.  The map's cells are uniform: unlike top_view_grid's there is no double-width cell at 0 and no
    extra row or column."""
    if isinstance(scale, (bool, np.bool_)) or not _integer(scale, "scale") >= 1:
        raise ValueError("scale must be a positive integer, got %r" % (scale,))
    (x0, x1), (y0, y1) = [(_integer(r[0], name), _integer(r[1], name)) for r, name in ((x_range, "x_range"), (y_range, "y_range"))]
    if not (x0 < x1 and y0 < y1):
        raise ValueError("x_range and y_range need lo < hi, got %r, %r" % (tuple(x_range), tuple(y_range)))
    if max(abs(x0), abs(x1), abs(y0), abs(y1)) > 2.0 ** 31:
        raise ValueError("x / y bounds must lie within +-2^31")
    s = int(scale)
    return occupancy_map_words(dict(top=int(x1) * s, left=int(y1) * s, rows=int(x1 - x0) * s, cols=int(y1 - y0) * s, scale=s, l_occ=l_occ, l_free=l_free,
                                    l_min=l_min, l_max=l_max))


def occupancy_pose(x, y, yaw):
    """float64 [..., 4] = (tx, ty, c, s): the pose of a frame whose vehicle axes stand at (x, y) in the world, turned by yaw (radians,
    counter-clockwise: towards +y, the left) - Pw = R Pf + t with R = [[c, -s], [s, c]], c = numpy.cos(yaw), s = numpy.sin(yaw)."""
    x, y, yaw = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64), np.asarray(yaw, np.float64))
    return np.stack([x, y, np.cos(yaw), np.sin(yaw)], -1)


def occupancy_map_centres(map):
    """(Xw float64 [rows], Yw float64 [cols]): the centres of the map's cells, (double)(2 (top - r) - 1) * half and (double)(2 (left - c)
    - 1) * half with half = 1.0 / (2 scale)."""
    w = occupancy_map_words(map)
    half = 1.0 / (2.0 * float(w["scale"]))
    return ((2 * (w["top"] - np.arange(w["rows"], dtype=np.int64)) - 1).astype(np.float64) * half,
            (2 * (w["left"] - np.arange(w["cols"], dtype=np.int64)) - 1).astype(np.float64) * half)


def occupancy_frame_grid(frame_grid):
    """(x_range, y_range, scale, rows, cols) of the grid the frames' states lie in - a dict with x_range, y_range, scale (z_range and
    occupancy_params' words where given) or an object with those attributes (engine.SvOccupancySpec, e.g. OccupancyResult.spec) - after
    occupancy_params' checks."""
    keys = ("x_range", "y_range", "z_range", "scale", "z_scale", "min_obstacle", "min_ground", "min_rays")
    if isinstance(frame_grid, dict):
        g = {k: frame_grid[k] for k in keys if k in frame_grid}
    else:
        g = {k: getattr(frame_grid, k) for k in keys if hasattr(frame_grid, k)}
    if not all(k in g for k in ("x_range", "y_range", "scale")):
        raise ValueError("the frame grid needs x_range, y_range and scale")
    g = {k: (tuple(v) if k.endswith("_range") else v) for k, v in g.items()}
    g.setdefault("z_range", (0, 1))  # plays no part here
    rows, cols, _ = occupancy_params(**g)
    return tuple(float(v) for v in g["x_range"]), tuple(float(v) for v in g["y_range"]), int(g["scale"]), rows, cols


def occupancy_scroll(a, shift, fill):
    """a read at (r + shift[0], c + shift[1]), `fill` where that lies outside: a new array."""
    rows, cols = a.shape
    dr, dc = int(shift[0]), int(shift[1])
    out = np.full_like(a, fill)
    r0, r1, c0, c1 = max(0, -dr), min(rows, rows - dr), max(0, -dc), min(cols, cols - dc)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = a[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def occupancy_fuse(state, poses, frame_grid, map, logodds=None, last_seen=None, seq0=0, shift=(0, 0)):
    """The definition of sv_occupancy_fuse_device: the states of B frames (uint8 [B, frame rows, frame cols], occupancy_grid's under
    frame_grid; one frame without B accepted) fused along their poses (float64 [B, 4] = (tx, ty, c, s), occupancy_pose) into the world
    map `map` (occupancy_map_params' words).  -> {"logodds": int16 [rows, cols], "last_seen": int32 [rows, cols] or None}, new arrays.

      map     logodds / last_seen coming in (None: a fresh map, 0 / -1; last_seen=False: none is kept) are read at (r + shift[0], c +
              shift[1]), 0 / -1 outside: `map` is the map going out, top_new = top_old - shift[0], left_new = left_old - shift[1].
      frame b dx = Xw - tx, dy = Yw - ty; Xf = c dx + s dy, Yf = c dy - s dx (every product and sum rounded on its own); a cell is seen iff
              fx0 < Xf < fx1 and fy0 < Yf < fy1, strictly - a pose with a word that is not finite fails this everywhere - and then takes
              the state st of frame cell (trunc(fx1 fs) - trunc(Xf fs), trunc(fy1 fs) - trunc(Yf fs)): 2 adds l_occ, 1 subtracts l_free,
              clamped to l_min .. l_max in int32; 0 and bytes above 2 leave the cell alone; st 1 or 2 sets last_seen = seq0 + b.
      order   b = 0 .. B - 1; because of the clamp it matters."""
    w = occupancy_map_words(map)
    (fx0, fx1), (fy0, fy1), fscale, frows, fcols = occupancy_frame_grid(frame_grid)
    rows, cols = w["rows"], w["cols"]
    st = np.asarray(state)
    if st.ndim == 2:
        st = st[None]
    if st.dtype != np.uint8 or st.ndim != 3 or st.shape[1:] != (frows, fcols):
        raise ValueError("state must be uint8 [B, %d, %d], got %s %s" % (frows, fcols, st.dtype, st.shape))
    B = st.shape[0]
    p = np.asarray(poses, np.float64)
    if p.ndim == 1 and B == 1:
        p = p[None]
    if p.shape != (B, 4):
        raise ValueError("poses must be float64 [%d, 4], got %s" % (B, p.shape))
    if B > OCCUPANCY_BATCH_MAX:
        raise ValueError("at most 65535 frames per call, got %d" % B)
    if isinstance(seq0, (bool, np.bool_)) or int(seq0) != seq0 or seq0 < 0 or int(seq0) + B > 2 ** 31 - 1:
        raise ValueError("seq0 must be an integer >= 0 with seq0 + B below 2^31, got %r" % (seq0,))
    if len(shift) != 2 or any(isinstance(v, (bool, np.bool_)) or int(v) != v or abs(int(v)) > 2 ** 31 - 1 for v in shift):
        raise ValueError("shift must be two integers (rows, cols), got %r" % (shift,))
    keep_seen = last_seen is not False
    L = np.zeros((rows, cols), np.int16) if logodds is None else np.asarray(logodds)
    S = np.full((rows, cols), -1, np.int32) if last_seen is None or not keep_seen else np.asarray(last_seen)
    if L.dtype != np.int16 or L.shape != (rows, cols) or S.dtype != np.int32 or S.shape != (rows, cols):
        raise ValueError("logodds must be int16 and last_seen int32 [%d, %d]" % (rows, cols))
    L = occupancy_scroll(L, shift, 0).astype(np.int32)
    S = occupancy_scroll(S, shift, -1)
    Xw, Yw = occupancy_map_centres(w)
    fs = float(fscale)
    FR1, FC1 = int(np.trunc(fx1 * fs)), int(np.trunc(fy1 * fs))
    for b in range(B):
        tx, ty, c, s = (np.float64(v) for v in p[b])
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = (Xw - tx)[:, None], (Yw - ty)[None, :]
            Xf, Yf = c * dx + s * dy, c * dy - s * dx
            seen = (Xf > fx0) & (Xf < fx1) & (Yf > fy0) & (Yf < fy1)
        fr = FR1 - np.trunc(Xf[seen] * fs).astype(np.int64)
        fc = FC1 - np.trunc(Yf[seen] * fs).astype(np.int64)
        cell = np.zeros((rows, cols), np.uint8)
        cell[seen] = st[b][fr, fc]
        L = np.where(cell == 2, np.clip(L + w["l_occ"], w["l_min"], w["l_max"]), np.where(cell == 1, np.clip(L - w["l_free"], w["l_min"], w["l_max"]), L))
        S = np.where((cell == 1) | (cell == 2), np.int32(int(seq0) + b), S)
    return {"logodds": L.astype(np.int16), "last_seen": S.astype(np.int32) if keep_seen else None}


def occupancy_pose_window(x, y, yaw, half, steps):
    """float64 [P, 3] = (x, y, yaw): the candidates of a window around the guess (x, y, yaw) - half = (dx, dy, dyaw), the window's half
    widths (metres, metres, radians; finite, >= 0), steps = (nx, ny, nyaw), odd integers >= 1 with P = nx ny nyaw <= 65535.  Row 0 is the
    guess itself, so that ties keep it; the other P - 1 follow in row-major (i, j, k) order over numpy.linspace(-half, +half, n) per axis
    (n = 1: the offset 0), the middle one - the guess - left out.  occupancy_pose turns the rows into poses."""
    g = [float(v) for v in (x, y, yaw)]
    if len(half) != 3 or len(steps) != 3:
        raise ValueError("half and steps must have three entries each, got %r, %r" % (half, steps))
    h = [float(v) for v in half]
    if not all(np.isfinite(v) for v in g + h) or min(h) < 0:
        raise ValueError("the guess and half must be finite and half >= 0, got %r, %r" % (g, h))
    for v in steps:
        if isinstance(v, (bool, np.bool_)) or int(v) != v or v < 1 or int(v) % 2 != 1:
            raise ValueError("steps must be odd integers >= 1, got %r" % (steps,))
    n = [int(v) for v in steps]
    if n[0] * n[1] * n[2] > OCCUPANCY_POSES_MAX:
        raise ValueError("a window of %d poses: at most 65535" % (n[0] * n[1] * n[2]))
    off = [np.linspace(-h[a], h[a], n[a]) if n[a] > 1 else np.zeros(1) for a in range(3)]
    grid = np.stack(np.meshgrid(g[0] + off[0], g[1] + off[1], g[2] + off[2], indexing="ij"), -1).reshape(-1, 3)
    mid = (n[0] // 2 * n[1] + n[1] // 2) * n[2] + n[2] // 2
    return np.concatenate([np.array([g]), grid[:mid], grid[mid + 1:]])


def occupancy_frame_points(frame_grid):
    """(Xf float64 [rows], Yf float64 [cols]): the point each row and each column of the frames' grid stands for in the match - with kx =
    trunc(fx1 fs) - fr, Xf = (double)(2 kx + sgn(kx)) * hf, hf = 1.0 / (2 fs): the middle of the cell, 0 for the double-width cell at 0;
    the same along y.  trunc(Xf fs) == kx: occupancy_fuse looks the point up in the same cell."""
    (_, fx1), (_, fy1), fscale, frows, fcols = occupancy_frame_grid(frame_grid)
    fs = float(fscale)
    hf = 1.0 / (2.0 * fs)
    kx = int(np.trunc(fx1 * fs)) - np.arange(frows, dtype=np.int64)
    ky = int(np.trunc(fy1 * fs)) - np.arange(fcols, dtype=np.int64)
    return (2 * kx + np.sign(kx)).astype(np.float64) * hf, (2 * ky + np.sign(ky)).astype(np.float64) * hf


def occupancy_match(state, poses, frame_grid, map, logodds, w_occ=1, w_free=0):
    """The definition of sv_map_match_device: the states of B frames (uint8 [B, frame rows, frame cols] under frame_grid; one frame
    without B accepted) scored against the world map `map` (occupancy_map_params' words) with its logodds (int16 [rows, cols]) at P
    candidate poses per frame (float64 [B, P, 4] = (tx, ty, c, s), occupancy_pose's; [P, 4] accepted for one frame).
    -> {"sums": int64 [B, P, 2] = (H, M), "counts": int32 [B, P, 2] = (n_occ, n_free), "score": int64 [B, P], "best": int32 [B],
        "best_score": int64 [B]}.

      point   frame cell (fr, fc) stands for (Xf[fr], Yf[fc]) of occupancy_frame_points.
      world   Xw = (c Xf - s Yf) + tx, Yw = (s Xf + c Yf) + ty, every product, difference and sum rounded on its own.
      map     gx = floor(Xw ms), gy = floor(Yw ms); the cell counts iff top - rows <= gx <= top - 1 and left - cols <= gy <= left - 1 - a
              pose with a word that is not finite fails this everywhere - and is map cell (top - 1 - gx, left - 1 - gy): the row rule of
              occupancy_recenter_shift.
      sums    H = the sum of logodds (as stored, not clamped) under the state-2 cells that count, n_occ their number; M and n_free the
              same for the state-1 cells, 0 with w_free == 0 (they are not visited).  Bytes 0 and above 2 play no part.
      score   w_occ H - w_free M, weights in 0 .. 32767 and not both 0; best = the lowest p with the largest score."""
    w = occupancy_map_words(map)
    _, _, _, frows, fcols = occupancy_frame_grid(frame_grid)
    rows, cols, top, left = w["rows"], w["cols"], w["top"], w["left"]
    st = np.asarray(state)
    if st.ndim == 2:
        st = st[None]
    if st.dtype != np.uint8 or st.ndim != 3 or st.shape[1:] != (frows, fcols):
        raise ValueError("state must be uint8 [B, %d, %d], got %s %s" % (frows, fcols, st.dtype, st.shape))
    B = st.shape[0]
    p = np.asarray(poses, np.float64)
    if p.ndim == 2 and B == 1:
        p = p[None]
    if p.ndim != 3 or p.shape[0] != B or p.shape[2] != 4:
        raise ValueError("poses must be float64 [%d, P, 4], got %s" % (B, p.shape))
    P = p.shape[1]
    if B > OCCUPANCY_BATCH_MAX or not 1 <= P <= OCCUPANCY_POSES_MAX or B * P >= 2 ** 31:
        raise ValueError("at most 65535 frames of 1 .. 65535 poses each and fewer than 2^31 in all, got %d x %d" % (B, P))
    for v in (w_occ, w_free):
        if isinstance(v, (bool, np.bool_)) or int(v) != v or not 0 <= v <= 32767:
            raise ValueError("w_occ and w_free must be integers in 0 .. 32767, got %r, %r" % (w_occ, w_free))
    w_occ, w_free = int(w_occ), int(w_free)
    if w_occ == 0 and w_free == 0:
        raise ValueError("w_occ and w_free must not both be 0")
    L = np.asarray(logodds)
    if L.dtype != np.int16 or L.shape != (rows, cols):
        raise ValueError("logodds must be int16 [%d, %d], got %s %s" % (rows, cols, L.dtype, L.shape))
    Xp, Yp = occupancy_frame_points(frame_grid)
    ms = float(w["scale"])
    sums, counts = np.zeros((B, P, 2), np.int64), np.zeros((B, P, 2), np.int32)
    for b in range(B):
        for slot, byte in ((0, 2), (1, 1)):
            if byte == 1 and w_free == 0:
                continue
            fr, fc = np.nonzero(st[b] == byte)
            if fr.size == 0:
                continue
            Xf, Yf = Xp[fr][None, :], Yp[fc][None, :]
            tx, ty, c, s = (p[b, :, k][:, None] for k in range(4))
            with np.errstate(invalid="ignore", over="ignore"):
                Xw, Yw = (c * Xf - s * Yf) + tx, (s * Xf + c * Yf) + ty
                gx, gy = np.floor(Xw * ms), np.floor(Yw * ms)
                inside = (gx >= top - rows) & (gx <= top - 1) & (gy >= left - cols) & (gy <= left - 1)
            r = np.where(inside, top - 1 - np.where(inside, gx, 0.0), 0).astype(np.int64)
            cc = np.where(inside, left - 1 - np.where(inside, gy, 0.0), 0).astype(np.int64)
            sums[b, :, slot] = np.where(inside, L[r, cc].astype(np.int64), 0).sum(1)
            counts[b, :, slot] = inside.sum(1)
    score = w_occ * sums[..., 0] - w_free * sums[..., 1]
    best = score.argmax(1).astype(np.int32)  # the first of the largest
    return {"sums": sums, "counts": counts, "score": score, "best": best, "best_score": score[np.arange(B), best] if B else np.zeros(0, np.int64)}


def occupancy_map_state(logodds, last_seen, occupied, free):
    """uint8, the shape of logodds: 2 where logodds >= occupied, else 1 where logodds <= free, both only in cells that were ever seen
    (last_seen >= 0), else 0 - OCCUPANCY_STATES' numbers."""
    L, S = np.asarray(logodds), np.asarray(last_seen)
    return np.where(S >= 0, np.where(L >= occupied, 2, np.where(L <= free, 1, 0)), 0).astype(np.uint8)


def occupancy_recenter_shift(map, x, y):
    """(shift_rows, shift_cols): the whole cells by which the map scrolls so that the world point (x, y) lies in its middle cell (rows //
    2, cols // 2).  Cell r spans (top - r - 1) / scale .. (top - r) / scale, so the point's row is top - 1 - floor(x scale); the map
    going out has top - shift_rows and left - shift_cols (ValueError where those leave +-2^24 or x, y are not finite)."""
    w = occupancy_map_words(map)
    if not (np.isfinite(x) and np.isfinite(y)):
        raise ValueError("recenter needs a finite point, got (%r, %r)" % (x, y))
    kx, ky = np.floor(float(x) * float(w["scale"])), np.floor(float(y) * float(w["scale"]))
    if max(abs(kx), abs(ky)) >= 2.0 ** 25:
        raise ValueError("the point (%r, %r) lies 2^24 cells or more from the world's origin" % (x, y))
    top, left = w["rows"] // 2 + 1 + int(kx), w["cols"] // 2 + 1 + int(ky)
    occupancy_map_words(dict(w, top=top, left=left))
    return w["top"] - top, w["left"] - left


CLEARANCE_RADIUS_MAX = 254  # cells: R^2 <= 64516 < CLEARANCE_FAR
CLEARANCE_FAR = 65535       # d2 of a cell with no source within R
CLEARANCE_DISCS_MAX = 64
CLEARANCE_PATHS_MAX = 65535


def _clearance_sources(logodds, radius, t_occ, last_seen, unknown):
    """The checks of sv_clearance_device -> (sources bool [rows, cols], R)."""
    L = np.asarray(logodds)
    if L.dtype != np.int16 or L.ndim != 2 or not (1 <= L.shape[0] <= 32768 and 1 <= L.shape[1] <= 32768):
        raise ValueError("logodds must be int16 [rows, cols] of 1 .. 32768 in either dimension, got %s %s" % (L.dtype, L.shape))
    for v, lo, hi, what in ((radius, 1, CLEARANCE_RADIUS_MAX, "radius"), (t_occ, -32768, 32767, "t_occ")):
        if isinstance(v, (bool, np.bool_)) or int(v) != v or not lo <= v <= hi:
            raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    if not isinstance(unknown, (bool, np.bool_)) and unknown not in (0, 1):
        raise ValueError("unknown must be 0 or 1, got %r" % (unknown,))
    src = L >= int(t_occ)
    if unknown:
        if last_seen is None:
            raise ValueError("unknown needs last_seen")
    if last_seen is not None:
        S = np.asarray(last_seen)
        if S.dtype != np.int32 or S.shape != L.shape:
            raise ValueError("last_seen must be int32 %s, got %s %s" % (L.shape, S.dtype, S.shape))
        if unknown:
            src = src | (S < 0)
    return src, int(radius)


def occupancy_clearance(logodds, radius, t_occ, last_seen=None, unknown=False):
    """The definition of sv_clearance_device: uint16 [rows, cols], per cell of a map (logodds int16 [rows, cols], last_seen int32 of the
    same shape or None) the squared distance in cells to the nearest source - a cell with logodds >= t_occ or, with unknown, last_seen < 0
    - as the minimum over all sources of (r - r')^2 + (c - c')^2; CLEARANCE_FAR where that exceeds radius^2 (radius in cells, 1 .. 254) or
    there is no source; 0 on a source.  Cells outside the map are no sources.  This is the separable form: g = the rows to the nearest
    source of the same column (255 beyond radius), then the minimum over dc of dc^2 + g[c + dc]^2.  A minimum of integers: every order
    and every decomposition gives the same bits (occupancy_clearance_brute is the all-pairs form)."""
    src, R = _clearance_sources(logodds, radius, t_occ, last_seen, unknown)
    rows, cols = src.shape
    at = np.arange(rows, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(src, at, -(1 << 20)), 0)          # the last source at or above
    below = np.minimum.accumulate(np.where(src, at, 1 << 20)[::-1], 0)[::-1]  # the first at or below
    g = np.minimum(at - above, below - at)
    g = np.where(g > R, 255, g)
    g2 = g * g  # 65025 > R^2 where there is none
    best = g2.copy()
    for dc in range(1, min(R, cols - 1) + 1):
        best[:, dc:] = np.minimum(best[:, dc:], g2[:, :-dc] + dc * dc)
        best[:, :-dc] = np.minimum(best[:, :-dc], g2[:, dc:] + dc * dc)
    return np.where(best > R * R, CLEARANCE_FAR, best).astype(np.uint16)


def occupancy_clearance_brute(logodds, radius, t_occ, last_seen=None, unknown=False):
    """occupancy_clearance as the minimum over all (cell, source) pairs, written out: for tests on small maps only."""
    src, R = _clearance_sources(logodds, radius, t_occ, last_seen, unknown)
    rows, cols = src.shape
    sr, sc = np.nonzero(src)
    out = np.full((rows, cols), CLEARANCE_FAR, np.int64)
    if sr.size:
        r, c = np.mgrid[0:rows, 0:cols]
        d = ((r[..., None] - sr) ** 2 + (c[..., None] - sc) ** 2).min(-1)
        out = np.where(d > R * R, CLEARANCE_FAR, d)
    return out.astype(np.uint16)


def clearance_discs(discs_m, scale):
    """A footprint given in metres -> (centres float64 [n, 2], r2 int32 [n]) as clearance_paths takes them: discs_m [n, 3] = (px, py,
    radius) in vehicle axes, scale = the map's cells per metre; r2 = ceil(radius scale)^2 - rounded up, the conservative side."""
    d = np.asarray(discs_m, np.float64)
    if d.ndim != 2 or d.shape[1] != 3 or not 1 <= d.shape[0] <= CLEARANCE_DISCS_MAX:
        raise ValueError("discs must be [n, 3] = (px, py, radius) with 1 <= n <= 64, got %s" % (d.shape,))
    if isinstance(scale, (bool, np.bool_)) or not _integer(scale, "scale") >= 1:
        raise ValueError("scale must be a positive integer, got %r" % (scale,))
    if not np.isfinite(d).all() or (d[:, 2] < 0).any():
        raise ValueError("disc centres and radii must be finite and the radii >= 0")
    cells = np.ceil(d[:, 2] * float(scale))
    if (cells > CLEARANCE_RADIUS_MAX).any():
        raise ValueError("a disc radius of more than 254 cells")
    return np.ascontiguousarray(d[:, :2]), (cells.astype(np.int64) ** 2).astype(np.int32)


def clearance_png(d2):
    """uint8, the shape of d2: the distance in whole cells, min(255, isqrt(d2)), 255 where d2 is CLEARANCE_FAR - what --clearance writes."""
    D = np.asarray(d2).astype(np.int64)
    root = np.floor(np.sqrt(D.astype(np.float64))).astype(np.int64)  # below 2^16: the double's root of a square is exact
    return np.where(D == CLEARANCE_FAR, 255, np.minimum(root, 255)).astype(np.uint8)


def _clearance_footprint(centres, r2, radius):
    """The checks of sv_clearance_paths_device on the footprint -> (centres float64 [n, 2], r2 int32 [n], R)."""
    if isinstance(radius, (bool, np.bool_)) or int(radius) != radius or not 1 <= radius <= CLEARANCE_RADIUS_MAX:
        raise ValueError("radius must be an integer in 1 .. 254, got %r" % (radius,))
    P = np.asarray(centres, np.float64)
    q = np.asarray(r2)
    if P.ndim != 2 or P.shape[1] != 2 or not 1 <= P.shape[0] <= CLEARANCE_DISCS_MAX:
        raise ValueError("centres must be float64 [n, 2] with 1 <= n <= 64, got %s" % (P.shape,))
    if q.shape != (P.shape[0],) or q.dtype.kind not in "iu":
        raise ValueError("r2 must be %d integers, got %s %s" % (P.shape[0], q.dtype, q.shape))
    if (q < 0).any() or (q > int(radius) ** 2).any():
        raise ValueError("every r2 must lie in 0 .. radius^2 = %d - beyond it a saturated cell would hide a hit - got %s" % (int(radius) ** 2, q.tolist()))
    return np.ascontiguousarray(P), q.astype(np.int32), int(radius)


def clearance_cells(map, poses, centres):
    """(inside bool [..., n], r int64 [..., n], c int64 [..., n]): the map cell each disc centre (float64 [n, 2], vehicle axes) falls into
    under each pose (float64 [..., 4] = (tx, ty, c, s)) - occupancy_match's arithmetic and cell rule; r and c are 0 where not inside."""
    w = occupancy_map_words(map)
    rows, cols, top, left, ms = w["rows"], w["cols"], w["top"], w["left"], float(w["scale"])
    p = np.asarray(poses, np.float64)[..., None, :]
    px, py = np.asarray(centres, np.float64)[:, 0], np.asarray(centres, np.float64)[:, 1]
    tx, ty, c, s = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    with np.errstate(invalid="ignore", over="ignore"):
        Xw, Yw = (c * px - s * py) + tx, (s * px + c * py) + ty
        gx, gy = np.floor(Xw * ms), np.floor(Yw * ms)
        inside = (gx >= top - rows) & (gx <= top - 1) & (gy >= left - cols) & (gy <= left - 1)
    r = np.where(inside, top - 1 - np.where(inside, gx, 0.0), 0).astype(np.int64)
    cc = np.where(inside, left - 1 - np.where(inside, gy, 0.0), 0).astype(np.int64)
    return inside, r, cc


def clearance_paths(d2, map, poses, centres, r2, radius):
    """The definition of sv_clearance_paths_device: K candidate paths of T poses each (float64 [K, T, 4] = (tx, ty, c, s), occupancy_pose's)
    checked against the field d2 (uint16 [rows, cols], occupancy_clearance's with `radius`) of the map `map` (occupancy_map_params' words)
    for a footprint of n discs (clearance_discs: centres float64 [n, 2] in vehicle axes, r2 int32 [n] squared radii in cells, each
    <= radius^2).  -> {"first_hit": int32 [K], "min_d2": int32 [K], "n_outside": int32 [K]}.

      world   Xw = (c px - s py) + tx, Yw = (s px + c py) + ty, every product, difference and sum rounded on its own.
      map     gx = floor(Xw ms), gy = floor(Yw ms); the lookup is inside iff top - rows <= gx <= top - 1 and left - cols <= gy <= left - 1
              - a pose with a word that is not finite is outside - and reads map cell (top - 1 - gx, left - 1 - gy): occupancy_match's.
      path    first_hit = the lowest step with an inside disc whose d2[cell] <= r2, T if none; min_d2 = the least d2[cell] over the
              inside lookups, CLEARANCE_FAR if none; n_outside = the (step, disc) lookups that were not inside."""
    w = occupancy_map_words(map)
    P, q, _ = _clearance_footprint(centres, r2, radius)
    D = np.asarray(d2)
    if D.dtype != np.uint16 or D.shape != (w["rows"], w["cols"]):
        raise ValueError("d2 must be uint16 [%d, %d], got %s %s" % (w["rows"], w["cols"], D.dtype, D.shape))
    p = np.asarray(poses, np.float64)
    if p.ndim != 3 or p.shape[2] != 4 or p.shape[0] > CLEARANCE_PATHS_MAX or not 1 <= p.shape[1] <= CLEARANCE_PATHS_MAX:
        raise ValueError("poses must be float64 [K, T, 4] with K <= 65535 and 1 <= T <= 65535, got %s" % (p.shape,))
    K, T = p.shape[:2]
    inside, r, cc = clearance_cells(w, p, P)
    v = np.where(inside, D[r, cc].astype(np.int64), CLEARANCE_FAR)
    hit = (inside & (v <= q)).any(-1)  # [K, T]
    first = np.where(hit.any(1), hit.argmax(1), T)
    return {"first_hit": first.astype(np.int32), "min_d2": v.reshape(K, -1).min(1).astype(np.int32) if K else np.zeros(0, np.int32),
            "n_outside": (~inside).reshape(K, -1).sum(1).astype(np.int32)}


COST_INF = 0x7FFFFFFF      # cost of a cell no goal reaches, and of a blocked cell
COST_BLOCKED = 255         # pen of a cell no path may enter
COST_PEN_MAX = 254         # the largest penalty of a free cell; also the largest soft and weight
COST_STEP_AXIAL, COST_STEP_DIAGONAL = 10, 14
COST_CELLS_MAX = 8000000   # (cells - 1) * (254 + 14) stays below 2^31 - 1
COST_GOALS_MAX = 1024
COST_ROUTES_MAX = 65535
COST_CAPACITY_MAX = 65535
COST_MOVES = ((-1, 0), (0, -1), (0, 1), (1, 0), (-1, -1), (-1, 1), (1, -1), (1, 1))  # a route's ties go to the first of these
ROUTE_GOAL, ROUTE_OUTSIDE, ROUTE_UNREACHABLE, ROUTE_CAPACITY, ROUTE_STUCK = 0, 1, 2, 3, 4  # cost_routes' status


def _cost_int(v, lo, hi, what):
    if isinstance(v, (bool, np.bool_)) or int(v) != v or not lo <= v <= hi:
        raise ValueError("%s must be an integer in %d .. %d, got %r" % (what, lo, hi, v))
    return int(v)


def cost_isqrt(v):
    """floor(sqrt(v)) of integers in 0 .. 65535, exactly: the compare ladder the kernel runs - bit 7 down to bit 0, a bit stays where
    the square of the root so far does not exceed v."""
    v = np.asarray(v).astype(np.int64)
    r = np.zeros_like(v)
    for b in (128, 64, 32, 16, 8, 4, 2, 1):
        t = r | b
        r = np.where(t * t <= v, t, r)
    return r


def cost_cells(d2, r2_block, soft=0, weight=0, radius=CLEARANCE_RADIUS_MAX):
    """The definition of sv_cost_cells_device: pen uint8, the shape of d2 (uint16 [rows, cols], occupancy_clearance's with `radius`) -
    COST_BLOCKED = 255 where d2 <= r2_block, elsewhere min(254, weight * max(0, soft - isqrt(d2))) with isqrt the floor of the root,
    and 0 where d2 is CLEARANCE_FAR.  0 <= r2_block <= radius^2: above it a saturated cell would hide an obstacle, as for
    clearance_paths' r2.  soft and weight in 0 .. 254."""
    D = np.asarray(d2)
    if D.dtype != np.uint16 or D.ndim != 2 or not (1 <= D.shape[0] <= 32768 and 1 <= D.shape[1] <= 32768):
        raise ValueError("d2 must be uint16 [rows, cols] of 1 .. 32768 in either dimension, got %s %s" % (D.dtype, D.shape))
    R = _cost_int(radius, 1, CLEARANCE_RADIUS_MAX, "radius")
    r2_block = _cost_int(r2_block, 0, R * R, "r2_block (0 .. radius^2: beyond it a saturated cell would hide an obstacle)")
    soft, weight = _cost_int(soft, 0, COST_PEN_MAX, "soft"), _cost_int(weight, 0, COST_PEN_MAX, "weight")
    v = D.astype(np.int64)
    pen = np.minimum(COST_PEN_MAX, weight * np.maximum(0, soft - cost_isqrt(v)))
    pen = np.where(v == CLEARANCE_FAR, 0, pen)
    return np.where(v <= r2_block, COST_BLOCKED, pen).astype(np.uint8)


def _cost_pen(pen):
    P = np.asarray(pen)
    if P.dtype != np.uint8 or P.ndim != 2 or not (1 <= P.shape[0] <= 32768 and 1 <= P.shape[1] <= 32768):
        raise ValueError("pen must be uint8 [rows, cols] of 1 .. 32768 in either dimension, got %s %s" % (P.dtype, P.shape))
    if P.shape[0] * P.shape[1] > COST_CELLS_MAX:
        raise ValueError("a field of %d x %d cells: at most %d, so that every cost stays below 2^31 - 1" % (P.shape + (COST_CELLS_MAX,)))
    return P


def _cost_cell_list(cells, lo, hi, what):
    g = np.asarray(cells)
    if g.dtype.kind not in "iu" or g.ndim != 2 or g.shape[1] != 2 or not lo <= g.shape[0] <= hi:
        raise ValueError("%s must be integers [n, 2] = (row, col) with %d <= n <= %d, got %s %s" % (what, lo, hi, g.dtype, g.shape))
    if g.size and (np.abs(g.astype(np.int64)) > 2 ** 31 - 1).any():
        raise ValueError("%s must fit int32" % what)
    return g.astype(np.int32)


def _cost_seeds(P, goals):
    """The goals that count: inside the map and on a free cell -> (rows int64 [n], cols int64 [n])."""
    g = _cost_cell_list(goals, 1, COST_GOALS_MAX, "goals").astype(np.int64)
    ok = (g[:, 0] >= 0) & (g[:, 0] < P.shape[0]) & (g[:, 1] >= 0) & (g[:, 1] < P.shape[1])
    g = g[ok]
    g = g[P[g[:, 0], g[:, 1]] != COST_BLOCKED]
    return g[:, 0], g[:, 1]


def _cost_admissible(P):
    """bool [8, rows, cols]: may a path step from cell a = (r, c) to a + COST_MOVES[k]?  Both cells free and, for a diagonal move, the
    two cells that share the corner as well; outside the map is blocked."""
    rows, cols = P.shape
    free = np.zeros((rows + 2, cols + 2), bool)
    free[1:-1, 1:-1] = P != COST_BLOCKED
    at = lambda dr, dc: free[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]  # noqa: E731
    return np.stack([at(0, 0) & at(dr, dc) & at(dr, 0) & at(0, dc) for dr, dc in COST_MOVES])


def cost_to_goal(pen, goals):
    """The definition of sv_cost_to_goal_device at its fixed point: int32 [rows, cols], per cell of a map with penalties pen (uint8,
    cost_cells' or the caller's own; 255 = blocked) the length of the cheapest path to the nearest goal.

      free    a cell inside the map with pen != 255.  Outside the map is blocked: here the map's edge is a wall.
      move    between 8-neighbours a and b, admissible iff both are free and, for a diagonal move, the two cells that share the corner -
              (a.r, b.c) and (b.r, a.c) - are free too: no corner is cut.  A step costs 10 along an axis and 14 diagonally.
      goals   integers [G, 2] = (row, col), 1 <= G <= 1024; a goal outside the map or on a blocked cell is ignored.
      cost    0 on every remaining goal; on any other free cell a, pen[a] + the minimum over the admissible b with a finite cost of
              cost[b] + step; COST_INF where there is none, and on blocked cells.

    The shortest-path length under strictly positive weights: unique, so every relaxation order that reaches a fixed point from the
    all-COST_INF start gives these bits.  This form is Dijkstra's with a heap; cost_to_goal_relax is the second derivation."""
    import heapq
    P = _cost_pen(pen)
    rows, cols = P.shape
    ok = [m.tolist() for m in _cost_admissible(P).reshape(8, -1)]  # plain lists over the flat cell index: the loop below is Python's
    pen_of = P.reshape(-1).tolist()
    moves = [(dr * cols + dc, COST_STEP_AXIAL if k < 4 else COST_STEP_DIAGONAL, ok[k]) for k, (dr, dc) in enumerate(COST_MOVES)]
    cost = [COST_INF] * (rows * cols)
    gr, gc = _cost_seeds(P, goals)
    heap = sorted(set((gr * cols + gc).tolist()))
    for a in heap:
        cost[a] = 0
    heap = [(0, a) for a in heap]
    while heap:
        d, a = heapq.heappop(heap)
        if d != cost[a]:
            continue
        for off, step, admissible in moves:  # admissibility is symmetric: b reaches a iff a reaches b
            if admissible[a]:
                b = a + off
                nd = d + step + pen_of[b]
                if nd < cost[b]:
                    cost[b] = nd
                    heapq.heappush(heap, (nd, b))
    return np.array(cost, np.int64).astype(np.int32).reshape(rows, cols)


def cost_relax_once(cost, pen, ok=None):
    """One whole-array Jacobi relaxation of cost_to_goal's rule: int64 [rows, cols], min(cost[a], pen[a] + min over the admissible b with
    a finite cost of cost[b] + step) per free cell a, every right-hand side read from `cost` as it was passed."""
    P = np.asarray(pen)
    ok = _cost_admissible(P) if ok is None else ok
    rows, cols = P.shape
    big = np.full((rows + 2, cols + 2), COST_INF, np.int64)
    big[1:-1, 1:-1] = cost
    best = np.full((rows, cols), COST_INF, np.int64)
    for k, (dr, dc) in enumerate(COST_MOVES):
        b = big[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]
        cand = b + (COST_STEP_AXIAL if k < 4 else COST_STEP_DIAGONAL) + P.astype(np.int64)
        best = np.minimum(best, np.where(ok[k] & (b != COST_INF), cand, COST_INF))
    return np.minimum(np.asarray(cost, np.int64), best)


def cost_to_goal_relax(pen, goals):
    """cost_to_goal by whole-array Jacobi relaxations from the all-COST_INF start until nothing changes: the second derivation of the
    same field, for tests on small maps."""
    P = _cost_pen(pen)
    ok = _cost_admissible(P)
    cost = np.full(P.shape, COST_INF, np.int64)
    gr, gc = _cost_seeds(P, goals)
    cost[gr, gc] = 0
    while True:
        new = cost_relax_once(cost, P, ok)
        if np.array_equal(new, cost):
            return cost.astype(np.int32)
        cost = new


def cost_routes(cost, pen, starts, capacity):
    """The definition of sv_cost_routes_device: K routes walked down the field `cost` (int32 [rows, cols], cost_to_goal's) of the map with
    penalties pen (uint8, the same shape), from starts (integers [K, 2] = (row, col), 0 <= K <= 65535), at most capacity (1 .. 65535)
    cells each.  -> {"cells": int16 [K, capacity, 2], "length": int32 [K], "status": int32 [K]}.

    From the start, repeat: write the current cell; stop with status 0 if its cost is 0; otherwise take, among the admissible neighbours
    (cost_to_goal's moves) with a finite cost, the one with the least cost[b] + step - ties go to the first in the order COST_MOVES.

      status 1   the start is outside the map; length 0.
      status 2   the start is blocked or its cost is COST_INF; length 0.
      status 4   the neighbour taken - if there is one - has no cost below the current cell's: the field was not converged.  The route
                 stops at the current cell and is kept.
      status 3   capacity cells were written before a goal was reached.

    Cells past length are -1.  On a converged field every step lowers the cost, so the walk ends; status 4 and capacity bound it on any
    other input."""
    P = _cost_pen(pen)
    C = np.asarray(cost)
    if C.dtype != np.int32 or C.shape != P.shape:
        raise ValueError("cost must be int32 %s, got %s %s" % (P.shape, C.dtype, C.shape))
    S = _cost_cell_list(starts, 0, COST_ROUTES_MAX, "starts")
    capacity = _cost_int(capacity, 1, COST_CAPACITY_MAX, "capacity")
    rows, cols = P.shape
    ok = _cost_admissible(P)
    K = S.shape[0]
    cells = np.full((K, capacity, 2), -1, np.int16)
    length, status = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for k in range(K):
        r, c = int(S[k, 0]), int(S[k, 1])
        if not (0 <= r < rows and 0 <= c < cols):
            status[k] = ROUTE_OUTSIDE
            continue
        if P[r, c] == COST_BLOCKED or C[r, c] == COST_INF:
            status[k] = ROUTE_UNREACHABLE
            continue
        n = 0
        while True:
            cells[k, n] = (r, c)
            n += 1
            here = int(C[r, c])
            if here == 0:
                status[k] = ROUTE_GOAL
                break
            best = None
            for m, (dr, dc) in enumerate(COST_MOVES):
                if ok[m, r, c] and C[r + dr, c + dc] != COST_INF:
                    v = int(C[r + dr, c + dc]) + (COST_STEP_AXIAL if m < 4 else COST_STEP_DIAGONAL)
                    if best is None or v < best[0]:
                        best = (v, r + dr, c + dc)
            if best is None or int(C[best[1], best[2]]) >= here:
                status[k] = ROUTE_STUCK
                break
            if n == capacity:
                status[k] = ROUTE_CAPACITY
                break
            r, c = best[1], best[2]
        length[k] = n
    return {"cells": cells, "length": length, "status": status}


def occupancy_cells_of(map, xy):
    """int32 [..., 2] = (row, col): the map cell each world point xy (float64 [..., 2] = (Xw, Yw), metres) falls into, by clearance_cells'
    rule - gx = floor(Xw ms), gy = floor(Yw ms), cell (top - 1 - gx, left - 1 - gy).  A point outside the map, or not finite, gives
    (-1, -1): a goal there is ignored, a route from there has status 1."""
    w = occupancy_map_words(map)
    p = np.asarray(xy, np.float64)
    if p.shape[-1:] != (2,):
        raise ValueError("xy must be [..., 2] = (Xw, Yw), got %s" % (p.shape,))
    ms = float(w["scale"])
    with np.errstate(invalid="ignore", over="ignore"):
        gx, gy = np.floor(p[..., 0] * ms), np.floor(p[..., 1] * ms)
        inside = (gx >= w["top"] - w["rows"]) & (gx <= w["top"] - 1) & (gy >= w["left"] - w["cols"]) & (gy <= w["left"] - 1)
    r = np.where(inside, w["top"] - 1 - np.where(inside, gx, 0.0), -1)
    c = np.where(inside, w["left"] - 1 - np.where(inside, gy, 0.0), -1)
    return np.stack([r, c], -1).astype(np.int32)


FRONTIER_CELLS_MAX = 8000000      # a linear index r * cols + c stays below 2^23
FRONTIER_INDEX_BITS = 23
FRONTIER_CAPACITY_MAX = 65535
FRONTIER_NEIGHBOURS = ((-1, 0), (0, -1), (0, 1), (1, 0))  # where a free cell looks for unknown space
FRONTIER_LINKS = ((0, -1), (-1, -1), (-1, 0), (-1, 1))    # W, NW, N, NE: with their opposites, the 8 neighbours that make a cluster


def frontier_cells(logodds, last_seen, occupied, free, pen=None):
    """The definition of sv_frontier_cells_device: uint8 [rows, cols] of 0 and 1 - 1 iff the cell's state (occupancy_map_state's, with
    these thresholds) is 1, pen is None or pen[r, c] != COST_BLOCKED (a cell the vehicle cannot stand on is not a goal), and at least one
    of its 4-neighbours lies inside the map and has state 0.  Cells outside the map are not unknown: the map's edge makes no frontier,
    as it is a wall for cost_to_goal; what lies beyond is gained by recentering the map."""
    L, S = np.asarray(logodds), np.asarray(last_seen)
    if L.dtype != np.int16 or L.ndim != 2 or not (1 <= L.shape[0] <= 32768 and 1 <= L.shape[1] <= 32768):
        raise ValueError("logodds must be int16 [rows, cols] of 1 .. 32768 in either dimension, got %s %s" % (L.dtype, L.shape))
    if S.dtype != np.int32 or S.shape != L.shape:
        raise ValueError("last_seen must be int32 %s, got %s %s" % (L.shape, S.dtype, S.shape))
    occupied, free = _cost_int(occupied, -2 ** 31, 2 ** 31 - 1, "occupied"), _cost_int(free, -2 ** 31, 2 ** 31 - 1, "free")
    rows, cols = L.shape
    state = occupancy_map_state(L.astype(np.int64), S, occupied, free)
    unknown = np.zeros((rows + 2, cols + 2), bool)  # False around the map
    unknown[1:-1, 1:-1] = state == 0
    near = np.zeros((rows, cols), bool)
    for dr, dc in FRONTIER_NEIGHBOURS:
        near |= unknown[1 + dr:1 + dr + rows, 1 + dc:1 + dc + cols]
    mask = (state == 1) & near
    if pen is not None:
        P = np.asarray(pen)
        if P.dtype != np.uint8 or P.shape != L.shape:
            raise ValueError("pen must be uint8 %s, got %s %s" % (L.shape, P.dtype, P.shape))
        mask &= P != COST_BLOCKED
    return mask.astype(np.uint8)


def _frontier_mask(mask, min_cells, capacity):
    M = np.asarray(mask)
    if M.dtype != np.uint8 or M.ndim != 2 or not (1 <= M.shape[0] <= 32768 and 1 <= M.shape[1] <= 32768):
        raise ValueError("mask must be uint8 [rows, cols] of 1 .. 32768 in either dimension, got %s %s" % (M.dtype, M.shape))
    if M.shape[0] * M.shape[1] > FRONTIER_CELLS_MAX:
        raise ValueError("a mask of %d x %d cells: at most %d, so that a linear index stays below 2^23" % (M.shape + (FRONTIER_CELLS_MAX,)))
    return M, _cost_int(min_cells, 1, FRONTIER_CELLS_MAX, "min_cells"), _cost_int(capacity, 1, FRONTIER_CAPACITY_MAX, "capacity")


def frontier_labels(mask):
    """int32, the shape of mask: -1 where mask is 0, elsewhere the least linear index r * cols + c of the cell's 8-connected component of
    non-zero cells.  A union-find over the whole array: every pair of linked members hooks the larger of its two roots under the
    smaller one, all chains are halved until they are flat, and both repeat until no linked pair has two roots.  Parents only ever
    descend, so a tree's root is the least index of its set: the label does not depend on the order of the unions."""
    M = np.asarray(mask) != 0
    rows, cols = M.shape
    index = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    pairs = []
    for dr, dc in FRONTIER_LINKS:
        c0, c1 = max(0, -dc), cols - max(0, dc)  # the cells a = (r, c) whose partner b = (r + dr, c + dc) is inside the map
        a, b = (slice(-dr, rows), slice(c0, c1)), (slice(0, rows + dr), slice(c0 + dc, c1 + dc))
        both = M[a] & M[b]
        pairs.append(np.stack([index[a][both], index[b][both]], 1))
    pairs = np.concatenate(pairs)
    parent = index.reshape(-1).copy()
    while True:
        ra, rb = parent[pairs[:, 0]], parent[pairs[:, 1]]  # roots: the chains are flat here
        apart = ra != rb
        if not apart.any():
            break
        pairs, ra, rb = pairs[apart], ra[apart], rb[apart]  # a pair once united stays so
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            up = parent[parent]
            if (up == parent).all():
                break
            parent = up
    return np.where(M, parent.reshape(rows, cols), -1).astype(np.int32)


def frontier_clusters(mask, min_cells=1, capacity=1024):
    """The definition of sv_frontier_clusters_device: mask uint8 [rows, cols] (a member is a non-zero byte; rows, cols in 1 .. 32768, rows
    * cols <= 8 000 000), min_cells in 1 .. 8 000 000, capacity in 1 .. 65535 -> dict of

      label     int32 [rows, cols]: frontier_labels'
      clusters  int32 [capacity, 8]: row k = (label, size, rep_r, rep_c, r0, c0, r1, c1) of the k-th component of at least min_cells
                members in ascending order of label - the order in which a scan of the map meets them; r0 .. c1 the inclusive bounding
                box; (rep_r, rep_c) the member nearest to the integer centroid cell cr = (2 sum_r + size) // (2 size), cc likewise
                (rounded half up: inside the box) by (r - cr)^2 + (c - cc)^2, ties to the least linear index.  Rows from min(kept,
                capacity) on are -1
      sums      int64 [capacity, 2]: (sum_r, sum_c) over the members of the row's component, 0 past the written rows
      info      int32 [4]: the kept components (above capacity: rows were dropped), all components, the members, the rows written."""
    M, min_cells, capacity = _frontier_mask(mask, min_cells, capacity)
    rows, cols = M.shape
    label = frontier_labels(M)
    clusters, sums = np.full((capacity, 8), -1, np.int32), np.zeros((capacity, 2), np.int64)
    at = np.flatnonzero(label.reshape(-1) >= 0).astype(np.int64)
    roots, which, size = np.unique(label.reshape(-1)[at], return_inverse=True, return_counts=True)  # ascending labels
    keep = size >= min_cells
    kept, members = int(keep.sum()), len(at)
    n = min(kept, capacity)
    rank = np.where(keep, np.cumsum(keep) - 1, -1)
    rank = np.where(rank < capacity, rank, -1)[which.reshape(-1)]  # per member; -1: its component has no row
    at, rank = at[rank >= 0], rank[rank >= 0]
    r, c = at // cols, at % cols
    if n:
        sum_r, sum_c, sz = np.zeros(n, np.int64), np.zeros(n, np.int64), size[keep][:n].astype(np.int64)
        np.add.at(sum_r, rank, r), np.add.at(sum_c, rank, c)
        box = np.stack([np.full(n, rows, np.int64), np.full(n, cols, np.int64), np.full(n, -1, np.int64), np.full(n, -1, np.int64)], 1)
        np.minimum.at(box[:, 0], rank, r), np.minimum.at(box[:, 1], rank, c), np.maximum.at(box[:, 2], rank, r), np.maximum.at(box[:, 3], rank, c)
        cr, cc = (2 * sum_r + sz) // (2 * sz), (2 * sum_c + sz) // (2 * sz)
        key = np.full(n, np.iinfo(np.int64).max, np.int64)
        np.minimum.at(key, rank, ((r - cr[rank]) ** 2 + (c - cc[rank]) ** 2) << FRONTIER_INDEX_BITS | at)
        rep = key & ((1 << FRONTIER_INDEX_BITS) - 1)
        clusters[:n] = np.concatenate([np.stack([roots[keep][:n], sz, rep // cols, rep % cols], 1), box], 1)
        sums[:n] = np.stack([sum_r, sum_c], 1)
    return {"label": label, "clusters": clusters, "sums": sums, "info": np.array([kept, len(roots), members, n], np.int32)}


def frontier_goals(map, clusters):
    """float64 [n, 2] = (Xw, Yw): the world centres (occupancy_map_centres) of the representatives of the written rows of clusters (int32
    [capacity, 8], frontier_clusters') - the points cost_to_goal takes as its goals."""
    C = np.asarray(clusters)
    if C.ndim != 2 or C.shape[1] != 8 or C.dtype.kind not in "iu":
        raise ValueError("clusters must be integers [capacity, 8], got %s %s" % (C.dtype, C.shape))
    Xw, Yw = occupancy_map_centres(map)
    C = C[C[:, 0] >= 0].astype(np.int64)
    return np.stack([Xw[C[:, 2]], Yw[C[:, 3]]], 1) if len(C) else np.zeros((0, 2), np.float64)


def frontier_lines(map, clusters, info):
    """What --frontiers prints: a line for the counts of info, then one per written row of clusters - rank, size, the representative's
    world centre in metres and the inclusive box in cells."""
    C = np.asarray(clusters)
    C = C[C[:, 0] >= 0]
    xy = frontier_goals(map, C)
    head = "frontiers: %d clusters kept of %d, %d cells, %d rows" % tuple(int(v) for v in np.asarray(info))
    return [head] + ["frontier %d: %d cells, representative (%r, %r) m, rows %d..%d, cols %d..%d" % (k, row[1], float(x), float(y), row[4], row[6], row[5], row[7])
                     for k, (row, (x, y)) in enumerate(zip(C.tolist(), xy))]


def frontier_png(label, clusters):
    """uint8, the shape of label: 0 on non-members and on members whose component has no row, 1 + (rank mod 255) on the members of the
    written row `rank` - what --frontiers writes."""
    L, C = np.asarray(label), np.asarray(clusters)
    roots = C[C[:, 0] >= 0, 0].astype(np.int64)
    out = np.zeros(L.shape, np.uint8)
    if len(roots):
        flat = L.reshape(-1).astype(np.int64)
        k = np.searchsorted(roots, np.maximum(flat, 0))  # the rows ascend by label
        hit = (flat >= 0) & (k < len(roots)) & (roots[np.minimum(k, len(roots) - 1)] == flat)
        out.reshape(-1)[hit] = (1 + k[hit] % 255).astype(np.uint8)
    return out


VIEW_REACH_MAX = 254    # cells a ray may span on either axis: the window of a candidate is at most 509 cells a side
VIEW_RAYS_MAX = 1024
VIEW_POSES_MAX = 65535  # candidates per call, G * P
VIEW_FULL, VIEW_HIT, VIEW_EDGE, VIEW_CORNER, VIEW_UNKNOWN, VIEW_INVALID = range(6)  # the status of a ray


def view_rays(fov, n_rays, range_m, scale):
    """(ends float64 [n_rays, 2], reach int): a fan of n_rays rays (1 .. 1024) over the field of view fov (radians, 0 < fov <= 2 pi) that
    reach range_m metres, for a map of `scale` cells per metre.  Ray j points at a_j = (j + 0.5) / n_rays * fov - fov / 2 - angle 0 is
    the vehicle's +x, angles grow counter-clockwise as occupancy_pose's yaw - and ends at range_m (cos a_j, sin a_j) in vehicle axes;
    reach = ceil(range_m scale) + 1 cells bounds the end of every ray from wherever in its cell the vehicle stands (ValueError above
    254).  The only trigonometry of the stage: it runs on the host."""
    if isinstance(n_rays, (bool, np.bool_)) or int(n_rays) != n_rays or not 1 <= n_rays <= VIEW_RAYS_MAX:
        raise ValueError("n_rays must be an integer in 1 .. 1024, got %r" % (n_rays,))
    if isinstance(scale, (bool, np.bool_)) or not np.isfinite(scale) or int(scale) != scale or scale < 1:
        raise ValueError("scale must be a positive integer, got %r" % (scale,))
    if not (np.isfinite(fov) and 0 < fov <= 2 * np.pi):
        raise ValueError("fov must lie in (0, 2 pi] radians, got %r" % (fov,))
    if not (np.isfinite(range_m) and range_m > 0):
        raise ValueError("range_m must be a positive number of metres, got %r" % (range_m,))
    reach = int(np.ceil(float(range_m) * int(scale))) + 1
    if reach > VIEW_REACH_MAX:
        raise ValueError("%r m are %d cells at scale %d, a reach of %d: at most 254" % (range_m, reach - 1, scale, reach))
    n = int(n_rays)
    a = (np.arange(n, dtype=np.float64) + 0.5) / n * float(fov) - float(fov) / 2
    return float(range_m) * np.stack([np.cos(a), np.sin(a)], 1), reach


def view_headings(xy, n):
    """float64 [len(xy), n, 4]: occupancy_pose of each point of xy (float64 [m, 2], world metres) at the n yaws 2 pi p / n."""
    p = np.asarray(xy, np.float64).reshape(-1, 2)
    if isinstance(n, (bool, np.bool_)) or int(n) != n or n < 1:
        raise ValueError("n must be a positive integer, got %r" % (n,))
    yaw = 2 * np.pi * np.arange(int(n), dtype=np.float64) / int(n)
    return occupancy_pose(p[:, None, 0], p[:, None, 1], yaw[None, :])


def _view_ray(S, r0, c0, r1, c1, max_unknown):
    """One valid ray through the states S from cell (r0, c0) towards cell (r1, c1) -> (status, the steps that are visible)."""
    rows, cols = S.shape
    r, c = occupancy_ray_cells(r0, c0, r1, c1, obstacle_end=False)  # the project's one line rule
    inside = (r >= 0) & (r < rows) & (c >= 0) & (c < cols)

    def states(rr, cc):  # 2 outside the map: the edge is a wall
        ok = (rr >= 0) & (rr < rows) & (cc >= 0) & (cc < cols)
        return np.where(ok, S[np.where(ok, rr, 0), np.where(ok, cc, 0)], 2)

    st = states(r, c)
    later = np.arange(len(r)) >= 1  # step 0 is the origin's cell: visible, and it never ends the ray
    corner = np.zeros(len(r), bool)
    corner[1:] = (r[1:] != r[:-1]) & (c[1:] != c[:-1]) & (states(r[:-1], c[1:]) == 2) & (states(r[1:], c[:-1]) == 2)
    edge = later & ~inside
    corner &= later & inside
    hit = later & inside & (st == 2)
    unknown = later & inside & (st == 0)
    spent = unknown & (np.cumsum(unknown) == max_unknown) if max_unknown > 0 else np.zeros(len(r), bool)
    stop = edge | corner | hit | spent
    if not stop.any():
        return VIEW_FULL, len(r)
    k = int(stop.argmax())
    if edge[k]:
        return VIEW_EDGE, k
    if corner[k]:
        return VIEW_CORNER, k
    return (VIEW_HIT if hit[k] else VIEW_UNKNOWN), k + 1


def occupancy_view(logodds, last_seen, map, poses, ends, reach, occupied, free, max_unknown=0):
    """The definition of sv_view_device: what the vehicle would see of the map (logodds int16 and last_seen int32 [rows, cols] with the
    words `map`) from each of the candidate poses (float64 [G, P, 4] = (tx, ty, c, s), G * P <= 65535) along the rays `ends` (float64
    [n_rays, 2], vehicle axes, metres) of at most `reach` cells (view_rays' pair), with the thresholds of occupancy_map_state and
    max_unknown in 0 .. 255 (0: no limit).  -> dict of counts int32 [G, P, 3] = (unknown, free, occupied), end_cells int16 [G, P, n_rays,
    2], status uint8 [G, P, n_rays], best int32 [G], best_score int32 [G].

      origin  gx = floor(tx ms), gy = floor(ty ms), cell (top - 1 - gx, left - 1 - gy): clearance_cells' rule.  A candidate with a word
              that is not finite or an origin outside the map is invalid: every ray VIEW_INVALID with end (-1, -1), counts 0, score -1.
      end     Xw = (c ex - s ey) + tx, Yw = (s ex + c ey) + ty, every product, difference and sum rounded on its own (clearance_paths'),
              and its cell by the same rule, not clipped to the map.  With (dr, dc) from the origin's cell to it, a ray is invalid on its
              own - VIEW_INVALID, end (-1, -1), it marks nothing - if its end is not finite or |dr| > reach or |dc| > reach.  Nothing is
              clamped: this guard is what bounds the window a candidate can see.
      walk    the steps k = 0 .. max(|dr|, |dc|) of occupancy_ray_cells(r0, c0, r1, c1, obstacle_end=False).  Step 0, the origin's cell,
              is visible and never ends the ray.  For k >= 1, in this order: cell k outside the map -> VIEW_EDGE, the cell not visible
              (the map's edge is a wall, as for cost_to_goal and frontier_cells); the step diagonal - both coordinates changed - and
              both side cells (r_prev, c), (r, c_prev) occupied or outside the map -> VIEW_CORNER, the cell not visible (a ray must not
              slip through a diagonal wall; one open side lets it pass); else cell k is visible, and its state 2 -> VIEW_HIT (occupied
              cells are seen and then stop the ray); its state 0 and it the max_unknown-th unknown cell among the steps k >= 1 of this
              ray, max_unknown > 0 -> VIEW_UNKNOWN (unknown cells are seen through, up to max_unknown).  A ray that reaches its last
              step is VIEW_FULL.  A ray's end cell is its last visible cell.
      counts  the DISTINCT visible cells of each state over all rays of the candidate: a cell crossed by fifty rays counts once.
      best    score = counts[..., 0], -1 for an invalid candidate; best[g] the lowest p with the largest score, best_score[g] that score."""
    w = occupancy_map_words(map)
    rows, cols, top, left, ms = w["rows"], w["cols"], w["top"], w["left"], float(w["scale"])
    L, Sn = np.asarray(logodds), np.asarray(last_seen)
    if L.dtype != np.int16 or L.shape != (rows, cols):
        raise ValueError("logodds must be int16 [%d, %d], got %s %s" % (rows, cols, L.dtype, L.shape))
    if Sn.dtype != np.int32 or Sn.shape != L.shape:
        raise ValueError("last_seen must be int32 %s, got %s %s" % (L.shape, Sn.dtype, Sn.shape))
    p, e = np.asarray(poses, np.float64), np.asarray(ends, np.float64)
    if p.ndim != 3 or p.shape[2] != 4 or p.shape[1] < 1 or p.shape[0] * p.shape[1] > VIEW_POSES_MAX:
        raise ValueError("poses must be float64 [G, P, 4] with P >= 1 and G * P <= 65535, got %s" % (p.shape,))
    if e.ndim != 2 or e.shape[1] != 2 or not 1 <= e.shape[0] <= VIEW_RAYS_MAX:
        raise ValueError("ends must be float64 [n_rays, 2] with 1 <= n_rays <= 1024, got %s" % (e.shape,))
    reach, max_unknown = _cost_int(reach, 1, VIEW_REACH_MAX, "reach"), _cost_int(max_unknown, 0, 255, "max_unknown")
    occupied, free = _cost_int(occupied, -2 ** 31, 2 ** 31 - 1, "occupied"), _cost_int(free, -2 ** 31, 2 ** 31 - 1, "free")
    S = occupancy_map_state(L.astype(np.int64), Sn, occupied, free)
    G, P, n_rays = p.shape[0], p.shape[1], e.shape[0]
    counts = np.zeros((G, P, 3), np.int32)
    end_cells = np.full((G, P, n_rays, 2), -1, np.int16)
    status = np.full((G, P, n_rays), VIEW_INVALID, np.uint8)
    score = np.full((G, P), -1, np.int32)
    tx, ty, c, s = (p[..., None, k] for k in range(4))
    with np.errstate(invalid="ignore", over="ignore"):
        gx0, gy0 = np.floor(tx * ms), np.floor(ty * ms)  # [G, P, 1]
        origin = np.isfinite(p).all(-1)[..., None] & (gx0 >= top - rows) & (gx0 <= top - 1) & (gy0 >= left - cols) & (gy0 <= left - 1)
        Xw, Yw = (c * e[:, 0] - s * e[:, 1]) + tx, (s * e[:, 0] + c * e[:, 1]) + ty  # [G, P, n_rays]
        gx1, gy1 = np.floor(Xw * ms), np.floor(Yw * ms)
        dr, dc = gx0 - gx1, gy0 - gy1  # rows and columns count against gx and gy
        valid = origin & np.isfinite(gx1) & np.isfinite(gy1) & (np.abs(dr) <= reach) & (np.abs(dc) <= reach)
    for g, q in zip(*np.nonzero(origin[..., 0])):
        r0, c0 = top - 1 - int(gx0[g, q, 0]), left - 1 - int(gy0[g, q, 0])
        seen = []
        for j in np.flatnonzero(valid[g, q]):
            r1, c1 = r0 + int(dr[g, q, j]), c0 + int(dc[g, q, j])
            status[g, q, j], m = _view_ray(S, r0, c0, r1, c1, max_unknown)
            r, cc = occupancy_ray_cells(r0, c0, r1, c1, obstacle_end=False, k_hi=m - 1)
            end_cells[g, q, j] = r[-1], cc[-1]
            seen.append(r * cols + cc)
        cells = np.unique(np.concatenate(seen)) if seen else np.zeros(0, np.int64)
        counts[g, q] = np.bincount(S.reshape(-1)[cells], minlength=3)[:3]
        score[g, q] = counts[g, q, 0]
    best = score.argmax(1).astype(np.int32) if G else np.zeros(0, np.int32)  # the first of the largest
    return {"counts": counts, "end_cells": end_cells, "status": status, "best": best,
            "best_score": score[np.arange(G), best] if G else np.zeros(0, np.int32)}


def view_ranges(map, poses, end_cells):
    """float64, the shape of end_cells without its last axis: the virtual range scan of a view - per ray the metres from the centre of
    the origin's cell (poses float64 [..., 4], the candidates of the view) to the centre of its end cell (end_cells [..., n_rays, 2],
    occupancy_view's), sqrt(dx dx + dy dy) over occupancy_map_centres; NaN for an invalid ray."""
    w = occupancy_map_words(map)
    E = np.asarray(end_cells).astype(np.int64)
    origin = occupancy_cells_of(w, np.asarray(poses, np.float64)[..., :2]).astype(np.int64)[..., None, :]
    Xw, Yw = occupancy_map_centres(w)
    on = (E[..., 0] >= 0) & (origin[..., 0] >= 0)
    dx = Xw[np.where(on, E[..., 0], 0)] - Xw[np.where(on, origin[..., 0], 0)]
    dy = Yw[np.where(on, E[..., 1], 0)] - Yw[np.where(on, origin[..., 1], 0)]
    return np.where(on, np.sqrt(dx * dx + dy * dy), np.nan)


def view_lines(poses_xyyaw, counts, best, best_score):
    """What --view prints: per frontier one line with its best arrival heading in degrees and the distinct cells seen from there -
    poses_xyyaw float64 [n, 3] (the best pose per frontier), counts [n, P, 3], best and best_score [n] (occupancy_view's)."""
    X, C, B, Sc = np.asarray(poses_xyyaw, np.float64), np.asarray(counts), np.asarray(best), np.asarray(best_score)
    lines = []
    for k in range(len(X)):
        if Sc[k] < 0:
            lines.append("view %d: no valid pose" % k)
        else:
            u, f, o = (int(v) for v in C[k, int(B[k])])
            lines.append("view %d: heading %r deg, sees %d unknown, %d free, %d occupied cells" % (k, float(np.degrees(X[k, 2])), u, f, o))
    return lines


class stereo_vision:
    def __init__(self, so_lib_path=DEFAULT_STEREO_VISION_SO_PATH, width=1242, height=375, defaultCalibFile=True, objectTracking=True,
                 graphics=False, display=False, scale=1, pc_extrapolation=1, YOLO_CFG="src/yolo/yolov4-tiny.cfg",
                 YOLO_WEIGHTS="src/yolo/yolov4-tiny.weights", YOLO_CLASSES="src/yolo/classes.txt",
                 CAMERA_CALIBRATION_YAML=DEFAULT_CALIBRATION, subsampling=False):
        if not os.path.exists(so_lib_path):
            raise FileNotFoundError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`" % so_lib_path)
        try:  # share one HIP runtime with PyTorch if the application also uses it (see engine.share_hip_runtime_with_torch)
            import torch  # noqa: F401
        except ImportError:
            pass
        self.sv = ctypes.CDLL(so_lib_path)
        self.width = width
        self.height = height
        self.sv.generatePointCloud.restype = ndpointer(dtype=ctypes.c_double, shape=(width * height, 3))
        self.defaultCalibFile = defaultCalibFile
        self.objectTracking = objectTracking
        self.graphics = graphics
        self.display = display
        self.scale = scale
        self.pc_extrapolation = pc_extrapolation
        self.YOLO_CFG = YOLO_CFG
        self.YOLO_WEIGHTS = YOLO_WEIGHTS
        self.YOLO_CLASSES = YOLO_CLASSES
        self.CAMERA_CALIBRATION_YAML = CAMERA_CALIBRATION_YAML
        self.subsampling = bool(subsampling)
        # reference: sv.py:180 - 14 entries (the C function declares 16, stereo_vision.cpp:566-581; the last two are never read here)
        self.sv.generatePointCloud.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_bool,
                                               ctypes.c_bool, ctypes.c_bool, ctypes.c_bool, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                               ctypes.c_char_p, ctypes.c_char_p]
        self.sv.sv_legacy_set_subsampling.argtypes = [ctypes.c_int]
        self.sv.sv_legacy_set_subsampling.restype = None
        self.sv.sv_legacy_set_subsampling(int(self.subsampling))  # frozen by the first frame, like the driver's static Elas (stereo_vision.cpp:307-311)
        self.sv.clean.restype = None
        self._closed = False
        self._bgra = None

    def generatePointCloud(self, left, right):
        left, right = np.asarray(left), np.asarray(right)
        if left.ndim != 3 or left.shape[2] != 3 or left.shape[:2] != (self.height, self.width) or right.shape != left.shape:
            raise ValueError("expected two BGR uint8 images of shape (%d, %d, 3)" % (self.height, self.width))
        # cv2.COLOR_BGR2BGRA: a fourth channel of 255.  Pillow's C loop does it in ~0.3 ms per image (the channel order is left
        # alone: "RGB" -> "RGBA" only appends alpha); plain numpy needs ~1.5 ms for the strided copy.  The library reads the
        # buffers during the call only.
        try:
            from PIL import Image
            self._bgra = (np.asarray(Image.fromarray(np.ascontiguousarray(left, dtype=np.uint8), "RGB").convert("RGBA")),
                          np.asarray(Image.fromarray(np.ascontiguousarray(right, dtype=np.uint8), "RGB").convert("RGBA")))
            self._bgra = tuple(np.ascontiguousarray(b) for b in self._bgra)
        except ImportError:
            if self._bgra is None or not self._bgra[0].flags.writeable:
                self._bgra = (np.full(left.shape[:2] + (4,), 255, np.uint8), np.full(left.shape[:2] + (4,), 255, np.uint8))
            self._bgra[0][:, :, :3] = left
            self._bgra[1][:, :, :3] = right
        try:
            return self.sv.generatePointCloud(self._bgra[0].ctypes.data, self._bgra[1].ctypes.data, self.CAMERA_CALIBRATION_YAML.encode("utf-8"), self.width, self.height, self.defaultCalibFile,
                                              self.objectTracking, self.graphics, self.display, self.scale, self.pc_extrapolation,
                                              self.YOLO_CFG.encode("utf-8"), self.YOLO_WEIGHTS.encode("utf-8"), self.YOLO_CLASSES.encode("utf-8"))
        except ValueError as e:  # NULL pointer from the library: initialisation or a HIP call failed (message on stderr)
            raise RuntimeError("generatePointCloud failed (see stderr)") from e

    def last_disparity_u8(self):
        """The reference's `dmap` of the last frame: uint8 (height, width), 4 x disparity (stereo_vision.cpp:316)."""
        w, h = ctypes.c_int(), ctypes.c_int()
        self.sv.sv_legacy_last_dmap.restype = ctypes.POINTER(ctypes.c_ubyte)
        p = self.sv.sv_legacy_last_dmap(ctypes.byref(w), ctypes.byref(h))
        return np.ctypeslib.as_array(p, shape=(h.value, w.value)).copy()

    def object_positions(self, boxes):
        """Mean (X, Y, Z) of the last frame's cloud inside each detector box [(x, y, w, h), ...] - what the reference's
        publishPointCloud computes for its tracked objects (stereo_vision.cpp:261-278); boxes come from your own detector."""
        b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
        out = np.zeros((b.shape[0], 3), np.float64)
        self.sv.sv_legacy_box_means.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        if self.sv.sv_legacy_box_means(b.ctypes.data, b.shape[0], out.ctypes.data) != 0:
            raise RuntimeError("no frame has been processed yet")
        return out

    def close(self):
        if not self._closed:
            self._closed = True
            self.sv.clean()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _imread_bgr(path, scale):
    from PIL import Image
    im = Image.open(path).convert("RGB")
    if scale != 1:
        im = im.resize((im.width // scale, im.height // scale), Image.BILINEAR)
    return np.asarray(im)[:, :, ::-1].copy()


def main(argv=None):
    parser = argparse.ArgumentParser(description="stereo_vision CLI for disparity calculation and 3D depth map generation from a stereo pair")
    parser.add_argument("-k", "--kitti", type=str, default="~/KITTI", help="Path to KITTI directory of test images")
    parser.add_argument("-s", "--subsampling", type=int, default=0, help="Set s=1 for evaluating only every second pixel")
    parser.add_argument("-f", "--scale", type=int, default=1, help="By what factor to scale down the image by")
    parser.add_argument("-p", "--pointcloud_interpolation", default=False, action="store_true", help="Interpolates the point cloud to the desired scale")
    parser.add_argument("-prl", "--parallel", default=False, action="store_true", help="Run parallel (this library is always the GPU build)")
    parser.add_argument("-d", "--demo", default=False, action="store_true", help="Run over the image_02/image_03 folders under --kitti")
    parser.add_argument("-dst", "--dataset", choices=["kitti2015", "kitti_smol"], default="kitti_smol", help="Dataset layout under --kitti")
    parser.add_argument("-c", "--camera_calibration", type=str, default=DEFAULT_CALIBRATION, help="OpenCV YAML calibration file")
    parser.add_argument("-o", "--object_track", default=False, action="store_true", help="(accepted for compatibility; no detector in this library)")
    parser.add_argument("-ycfg", "--yolo_cfg", type=str, default="", help="YOLO CFG file")
    parser.add_argument("-yw", "--yolo_weights", type=str, default="", help="YOLO Weights file")
    parser.add_argument("-ycl", "--yolo_classes", type=str, default="", help="YOLO Classes to track")
    parser.add_argument("-ctu", "--camera_to_use", default=-1, type=int, help="(cameras need cv2; not available)")
    parser.add_argument("-sw", "--swap", default=False, action="store_true", help="Swaps cameras")
    parser.add_argument("-n", "--frames", type=int, default=0, help="stop after this many frames (0 = all)")
    parser.add_argument("--batch", type=int, default=0, help="run the folder through a StereoRig in batches of N pairs and print pairs/s")
    parser.add_argument("--out", type=str, default="", help="write the 8-bit disparity maps (4 x disparity) as PNGs into this directory")
    parser.add_argument("--rectify", default=False, action="store_true", help="rectify the images before matching (both paths)")
    parser.add_argument("--top-view", type=str, default="", metavar="DIR",
                        help="with --batch: write each frame's bird's-eye view (points_2_top_view, mode 'reference') as a PNG into DIR: "
                             "the float disparity reprojected in metres (pixels with d <= 0 skipped), camera (right, down, forward) -> "
                             "(forward, left, up) by XR = [[0,0,1],[-1,0,0],[0,-1,0]], XT = 0; x 0..40, y -20..20, z -1.4..1.0, "
                             "scale 10 (401 x 401 cells, row 0 = 40 m ahead, column 0 = 20 m to the left)")
    parser.add_argument("--ply", type=str, default="", metavar="DIR",
                        help="with --batch: write each frame's coloured point cloud as DIR/<name>.ply (binary little-endian; float x y z, "
                             "uchar red green blue): the float disparity reprojected in metres, the axes and the crop of --top-view "
                             "(forward 0..40, left -20..20, up -1.4..1.0)")
    parser.add_argument("--voxel", type=float, default=0.0, metavar="METRES",
                        help="with --batch --ply: write the voxel-grid downsampled cloud instead - per occupied cube of this edge inside the "
                             "same crop one vertex, the centroid of its points with their mean colour")
    parser.add_argument("--voxel-map", type=str, default="", metavar="FILE.ply",
                        help="with --batch --ply --voxel --poses: fuse the frames' voxel clouds along the poses into one world-fixed voxel map "
                             "of the same edge and write it as one PLY of the whole drive: per occupied cube the centroid and the mean "
                             "colour of everything the drive saw in it, ordered by cell")
    parser.add_argument("--voxel-window", action="store_true",
                        help="with --voxel-map: let the map's box follow the vehicle - before a batch is inserted, the box is recentred by whole "
                             "cells on the pose of the batch's first frame (x and y) when that has left the middle third of the box on an axis; "
                             "voxels that leave the box are lost")
    parser.add_argument("--voxel-forget", type=int, default=0, metavar="FRAMES",
                        help="with --voxel-map: after every batch forget the voxels that none of the last FRAMES frames has seen")
    parser.add_argument("--voxel-carve", type=str, default="", metavar="REACH_M[,MIN_MISS[,RATIO]]",
                        help="with --voxel-map: after every batch's insert, carve the map along the batch's sight lines - a ray from the "
                             "camera's centre to every voxel row within REACH_M metres (at most 1023 cells); a voxel that none of the "
                             "batch's frames from the casting one on has seen, with at least MIN_MISS (default 2) rows' weight of rays "
                             "through it and at least RATIO / 256 (default 0) of its own weight, is emptied.  Prints rays, steps, touched "
                             "and carved per batch")
    parser.add_argument("--voxel-render", type=str, default="", metavar="DIR[,TOL_PX]",
                        help="with --voxel-map: before a batch is inserted, render the map built so far into the camera at the batch's "
                             "poses and compare the expected disparity with the batch's measured one at TOL_PX pixels (default 1); "
                             "writes per frame DIR/NNNNNN.expected.png (the model's colours) and DIR/NNNNNN.change.png (none, measured "
                             "only, expected only, agree, nearer = new, farther = seen through) and prints the pixels per label")
    parser.add_argument("--voxel-flatten", type=str, default="", metavar="X0,X1,Y0,Y1,SCALE[,STEP_M[,HEIGHT_M]]",
                        help="with --voxel-map: at the end of the run, flatten the voxel map into a flat map over X0 .. X1 by Y0 .. Y1 metres "
                             "(whole numbers; write --voxel-flatten=-5,45,... for a negative X0) at SCALE cells per metre - a voxel less than STEP_M (default 0.2) from the lowest voxel "
                             "within 2 cells is ground, one below HEIGHT_M (default 2) an obstacle, one above it overhead and no obstacle - "
                             "and write logodds, last_seen, floor, top and the map's words (map_top, map_left, ...: `top` is a plane here) to "
                             "<FILE without extension>.flat.npz; with "
                             "--clearance and --goal also the clearance field of that map (.flat.clearance.png) and the route from where "
                             "the drive ended (.flat.route.txt)")
    parser.add_argument("--voxel-clusters", type=str, default="", metavar="MIN_VOXELS[,CONNECTIVITY[,H_LO_M,H_HI_M]]",
                        help="with --voxel-map: at the end of the run, the connected components of the voxel map (CONNECTIVITY 6, 18 or 26, "
                             "default 26) with at least MIN_VOXELS voxels, among the voxels H_LO_M .. H_HI_M metres above the floor: the "
                             "box's without --voxel-flatten (default: every height), with it that flat map's local floor (default: its "
                             "STEP_M .. HEIGHT_M, the obstacle voxels, so the ground does not join the objects).  Writes <FILE without "
                             "extension>.clusters.txt, a line per cluster - least key, voxels, centre, box corners, first and last frame - "
                             "and .clusters.ply, the clustered voxels coloured by cluster")
    parser.add_argument("--voxel-match", type=str, default="", metavar="DX,DY,DZ,DYAW[,NX,NY,NZ,NYAW]",
                        help="with --voxel-map: take the poses as guesses at height 0 - frame 0 is inserted where its line says; every later "
                             "frame's voxel cloud is first matched against the voxel map built so far over a window of +-DX, +-DY, +-DZ metres "
                             "and +-DYAW radians around its line (NX x NY x NZ x NYAW poses, odd, default 5,5,3,5; the line itself wins ties) "
                             "and inserted at the best pose.  The refined poses are written next to FILE.ply as <FILE without "
                             ".ply>.poses.txt, one 'x y z yaw' per frame")
    parser.add_argument("--voxel-align", type=str, default="", metavar="ROUNDS[,MAX_DIST_CELLS[,DOF[,point|plane]]]",
                        help="with --voxel-map: before a batch's frames are inserted, refine their poses - the lines of --poses, or what "
                             "--voxel-match made of them - by at most ROUNDS rounds of iterative closest point against the voxel map built "
                             "so far: every row is paired with the nearest voxel within MAX_DIST_CELLS cells (default 1) and the pairs are "
                             "fitted in closed form, DOF 6 (default: roll and pitch as well) or 4 (yaw and the translation); 'plane' as the "
                             "fourth field fits the rows to the planes of the voxels' normals instead of to their means (default: point).  The refined "
                             "poses are written next to FILE.ply as <FILE without .ply>.aligned.txt, twelve words per frame: the rotation "
                             "row-major, then the translation")
    parser.add_argument("--occupancy", type=str, default="", metavar="DIR",
                        help="with --batch: write each frame's occupancy grid as a PNG into DIR (0 unknown, 127 free, 255 occupied): ground "
                             "plane and obstacle labels from the float disparity, then per cell of the grid of --top-view (vehicle axes) the "
                             "ground and obstacle pixels and the sight lines that crossed it")
    parser.add_argument("--occupancy-map", type=str, default="", metavar="FILE",
                        help="with --batch and --poses: fuse the frames' occupancy grids (those of --occupancy) along the poses into one "
                             "world-fixed log-odds map of 10 cells per metre and write its final state as a PNG (0 unknown, 127 free, 255 "
                             "occupied; row 0 = the largest x, column 0 = the largest y); the map covers the trajectory's bounding box "
                             "plus the reach of a frame's grid")
    parser.add_argument("--poses", type=str, default="", metavar="FILE",
                        help="for --occupancy-map and --voxel-map: a text file with one line 'x y yaw' per frame - the vehicle in the world, metres and "
                             "radians, yaw counter-clockwise")
    parser.add_argument("--odometry", type=str, default="", metavar="FILE",
                        help="with --batch: stereo visual odometry of the folder, before anything else runs - every frame matched against "
                             "the one before it and the camera's motion fitted (StereoRig.odometry, the batches overlapping by a frame).  "
                             "The chained poses are written to FILE, one line 'x y yaw' per frame as --poses reads them, frame 0 at the "
                             "origin, and the motions to <FILE>.rel.txt, twelve words per pair of frames: the rotation row by row, then "
                             "the translation, previous camera to current camera.  Without --poses the run takes FILE as its --poses")
    parser.add_argument("--tracks", type=str, default="", metavar="FILE",
                        help="with --batch and --odometry: the objects of every frame (StereoRig.objects' boxes) linked to those of the frame "
                             "before it by the odometry's matches and followed through the folder (StereoRig.track on the odometry's batches, "
                             "ObjectTracks at 10 frames a second); writes one line per frame and track to FILE: 'frame id x y w h X Y Z vx vy vz "
                             "n moving' - the box in pixels, its position in metres and its own velocity in m/s in the camera's axes (nan "
                             "until a motion is known), the matches behind the last motion, and whether it moves")
    parser.add_argument("--places", type=str, default="", metavar="FILE[,MIN_GAP[,ACCEPT]]",
                        help="with --voxel-map: place recognition (rig.PlaceIndex) - every frame's voxel rows get a polar height descriptor, "
                             "which is searched among the frames at least MIN_GAP (default 50) before it under every rotation and then "
                             "stored; a best candidate with 256 sad <= ACCEPT norm (default 64) writes one line to FILE: 'frame key shift "
                             "sad norm yaw_deg' - the frame it recognised, the shift in sectors and the heading against that frame in degrees")
    parser.add_argument("--pose-graph", type=str, default="", metavar="OUT[,ROUNDS[,GATE]]",
                        help="with --places: at the end of the run, the pose graph of the drive (rig.PoseGraph) - the chain of --poses or "
                             "--odometry, and a loop edge per frame that recognised an earlier one: the relative pose of the two as "
                             "--voxel-match and --voxel-align refined them where those are given, else the two at one place under the "
                             "recognised heading - optimised in ROUNDS rounds (default 10), a loop edge whose chi2 exceeds GATE switched "
                             "off (default: none); writes the corrected poses to OUT, twelve words a line (R row-major, then t): a file "
                             "--voxel-repose takes")
    parser.add_argument("--voxel-repose", type=str, default="", metavar="CORRECTED_POSES",
                        help="with --voxel-map: at the end of the run, re-pose the map from the poses its frames were inserted at to those of "
                             "CORRECTED_POSES - a file as --poses takes or --pose-graph writes, the result of a pose graph or of loop_spread - (rig.VoxelMap.repose: "
                             "every voxel moved by the correction of the frame that saw it last, into the box of the corrected "
                             "trajectory); writes <FILE>.reposed.ply beside the map and prints the counts")
    parser.add_argument("--temporal", type=str, default="", metavar="DIR[,TOL_PX[,MODE]]",
                        help="with --batch and --odometry: every frame's disparity map compared with the map of the frame before it, warped "
                             "under the fitted motion (StereoRig.temporal, on the odometry's batches: the front end and engine run once "
                             "more for it) at TOL_PX pixels (default 1), MODE fill (default), confirm or reject; writes per frame "
                             "DIR/NNNNNN.change.png (none, measured only, expected only, agree, nearer, farther) and DIR/NNNNNN.temporal.png "
                             "(the filtered map as the 8-bit disparity image) and prints the pixels per label of each batch")
    parser.add_argument("--match", type=str, default="", metavar="DX,DY,DYAW[,NX,NY,NYAW]",
                        help="with --occupancy-map and --poses: take the poses as guesses - frame 0 is fused where its line says; every later "
                             "frame is first matched against the map built so far over a window of +-DX, +-DY metres and +-DYAW radians "
                             "around its line (NX x NY x NYAW poses, odd, default 7,7,5; the line itself wins ties) and fused at the best "
                             "pose.  The refined poses are written next to FILE as <FILE without .png>.poses.txt, one 'x y yaw' per frame")
    parser.add_argument("--clearance", type=float, default=0.0, metavar="METRES",
                        help="with --occupancy-map: also write the final map's clearance field next to FILE as <FILE without "
                             ".png>.clearance.png, 8 bits, in FILE's orientation: per cell the distance in whole cells to the nearest "
                             "occupied cell (rounded down, at most 255), 255 beyond METRES")
    parser.add_argument("--goal", type=str, default="", metavar="X,Y",
                        help="with --occupancy-map, --poses and --clearance: after the drive, the cost-to-goal field of the final map "
                             "towards the world point (X, Y) in metres - cells within --clearance's METRES of an obstacle are blocked - "
                             "and the route from the last pose, written next to FILE as route.txt, one 'row col x y' line per cell; "
                             "prints the route's status, its length and the cost at its start")
    parser.add_argument("--frontiers", type=int, default=0, metavar="MIN_CELLS",
                        help="with --occupancy-map, --poses and --clearance: after the drive, the frontier clusters of the final map - the "
                             "free cells that touch undecided space and lie at least --clearance's METRES from an obstacle, in 8-connected "
                             "clusters of at least MIN_CELLS cells; prints one line per cluster (size, representative in metres, box) and "
                             "writes the label image next to FILE as <FILE without .png>.frontiers.png: 0, or 1 + (rank mod 255) on a "
                             "cluster's cells.  Without --goal the representatives are the goals of the cost-to-goal field and the route")
    parser.add_argument("--view", type=str, default="", metavar="FOV_DEG,RANGE_M[,RAYS[,HEADINGS]]",
                        help="with --frontiers: the best arrival heading per frontier - from each cluster's representative, HEADINGS yaws "
                             "(default 16) of a fan of RAYS rays (default 128) over FOV_DEG degrees that reach RANGE_M metres are cast "
                             "through the final map; prints per frontier the heading in degrees that sees the most undecided cells and "
                             "the distinct unknown, free and occupied cells seen from there")
    args = parser.parse_args(argv)
    if args.odometry and not args.batch:
        parser.error("--odometry needs --batch")
    if args.odometry and not args.poses and (args.occupancy_map or args.voxel_map):
        args.poses = args.odometry  # written below, before anything reads it
    if args.tracks and (not args.batch or not args.odometry):
        parser.error("--tracks needs --batch and --odometry")
    args.places_spec = None
    if args.places:
        if not args.voxel_map:
            parser.error("--places needs --voxel-map")
        try:
            args.places_spec = cli_places_spec(args.places)
        except ValueError as e:
            parser.error("--places: %s" % e)
    args.pose_graph_spec = None
    if args.pose_graph:
        if not args.places:
            parser.error("--pose-graph needs --places: the loops are the frames it recognises")
        try:
            args.pose_graph_spec = cli_pose_graph_spec(args.pose_graph)
        except ValueError as e:
            parser.error("--pose-graph: %s" % e)
    args.temporal_spec = None
    if args.temporal:
        if not args.batch or not args.odometry:
            parser.error("--temporal needs --batch and --odometry")
        try:
            args.temporal_spec = cli_temporal_spec(args.temporal)
        except ValueError as e:
            parser.error("--temporal: %s" % e)
    args.match_window = None
    args.voxel_match_window = None
    args.voxel_carve_spec = None
    args.goal_xy = None
    args.view_spec = None
    if args.view:
        if not args.frontiers:
            parser.error("--view needs --frontiers")
        try:
            words = args.view.split(",")
            fov_deg, range_m = float(words[0]), float(words[1])
            rays, headings = (int(words[2]) if len(words) > 2 else 128), (int(words[3]) if len(words) > 3 else 16)
            if len(words) > 4 or headings < 1 or headings > VIEW_POSES_MAX:
                raise ValueError
            view_rays(np.radians(fov_deg), rays, range_m, CLI_TOP_VIEW["scale"])
        except (ValueError, IndexError):
            parser.error("--view: FOV_DEG in (0, 360], RANGE_M > 0 of at most 253 cells, RAYS in 1 .. 1024, HEADINGS >= 1, got %r" % (args.view,))
        args.view_spec = (np.radians(fov_deg), range_m, rays, headings)
    if args.frontiers:
        if not (args.occupancy_map and args.poses and args.clearance):
            parser.error("--frontiers needs --occupancy-map, --poses and --clearance")
        if not 1 <= args.frontiers <= FRONTIER_CELLS_MAX:
            parser.error("--frontiers: MIN_CELLS in 1 .. %d, got %d" % (FRONTIER_CELLS_MAX, args.frontiers))
    if args.goal:
        if not (args.occupancy_map and args.poses and args.clearance):
            parser.error("--goal needs --occupancy-map, --poses and --clearance")
        try:
            args.goal_xy = tuple(float(w) for w in args.goal.split(","))
            if len(args.goal_xy) != 2 or not np.isfinite(args.goal_xy).all():
                raise ValueError("not two finite numbers")
        except ValueError as e:
            parser.error("--goal: X,Y in metres (%s)" % e)
    if args.clearance:
        if not args.occupancy_map:
            parser.error("--clearance needs --occupancy-map")
        if not (np.isfinite(args.clearance) and 0 < args.clearance and np.ceil(args.clearance * CLI_TOP_VIEW["scale"]) <= CLEARANCE_RADIUS_MAX):
            parser.error("--clearance: 1 .. 254 cells of %g m, got %r m" % (1.0 / CLI_TOP_VIEW["scale"], args.clearance))
    if args.match:
        if not args.occupancy_map:
            parser.error("--match needs --occupancy-map and --poses")
        try:
            words = args.match.split(",")
            if len(words) not in (3, 6):
                raise ValueError("%d words, not DX,DY,DYAW[,NX,NY,NYAW]" % len(words))
            args.match_window = (tuple(float(w) for w in words[:3]), tuple(int(w) for w in words[3:]) or (7, 7, 5))
            occupancy_pose_window(0.0, 0.0, 0.0, *args.match_window)
        except ValueError as e:
            parser.error("--match: %s" % e)
    if args.voxel_match:
        if not args.voxel_map:
            parser.error("--voxel-match needs --voxel-map")
        try:
            words = args.voxel_match.split(",")
            if len(words) not in (4, 8):
                raise ValueError("%d words, not DX,DY,DZ,DYAW[,NX,NY,NZ,NYAW]" % len(words))
            args.voxel_match_window = (tuple(float(w) for w in words[:4]), tuple(int(w) for w in words[4:]) or (5, 5, 3, 5))
            voxel_map_pose_window(0.0, 0.0, 0.0, 0.0, *args.voxel_match_window)
        except ValueError as e:
            parser.error("--voxel-match: %s" % e)
    args.voxel_align_spec = None
    if args.voxel_align:
        if not args.voxel_map:
            parser.error("--voxel-align needs --voxel-map")
        try:
            args.voxel_align_spec = cli_voxel_align_spec(args.voxel_align)
        except ValueError as e:
            parser.error("--voxel-align: %s" % e)
    if args.voxel_carve:
        if not args.voxel_map:
            parser.error("--voxel-carve needs --voxel-map")
        try:
            words = args.voxel_carve.split(",")
            if not 1 <= len(words) <= 3:
                raise ValueError("%d words, not REACH_M[,MIN_MISS[,RATIO]]" % len(words))
            args.voxel_carve_spec = cli_voxel_carve_spec(float(words[0]), int(words[1]) if len(words) > 1 else 2, int(words[2]) if len(words) > 2 else 0, args.voxel)
        except ValueError as e:
            parser.error("--voxel-carve: %s" % e)
    args.voxel_flatten_spec = None
    if args.voxel_flatten:
        if not args.voxel_map:
            parser.error("--voxel-flatten needs --voxel-map")
        try:
            args.voxel_flatten_spec = cli_voxel_flatten_spec(args.voxel_flatten, args.voxel)
        except ValueError as e:
            parser.error("--voxel-flatten: %s" % e)
    args.voxel_clusters_spec = None
    if args.voxel_clusters:
        if not args.voxel_map:
            parser.error("--voxel-clusters needs --voxel-map")
        try:
            args.voxel_clusters_spec = cli_voxel_clusters_spec(args.voxel_clusters, args.voxel)
        except ValueError as e:
            parser.error("--voxel-clusters: %s" % e)
    args.voxel_render_spec = None
    if args.voxel_render:
        if not args.voxel_map:
            parser.error("--voxel-render needs --voxel-map")
        try:
            args.voxel_render_spec = cli_voxel_render_spec(args.voxel_render)
        except ValueError as e:
            parser.error("--voxel-render: %s" % e)
    if args.voxel_repose and not args.voxel_map:
        parser.error("--voxel-repose needs --voxel-map")
    if (args.voxel_window or args.voxel_forget) and not args.voxel_map:
        parser.error("--voxel-window and --voxel-forget need --voxel-map")
    if args.voxel_forget < 0:
        parser.error("--voxel-forget: FRAMES >= 1, got %d" % args.voxel_forget)
    if args.occupancy_map and not args.poses:
        parser.error("--occupancy-map and --poses go together")
    if args.poses and not (args.occupancy_map or args.voxel_map):
        parser.error("--poses needs --occupancy-map or --voxel-map")
    if args.voxel_map and not (args.batch and args.ply and args.voxel and args.poses):
        parser.error("--voxel-map needs --batch, --ply, --voxel and --poses")
    if args.occupancy_map and not args.batch:
        parser.error("--occupancy-map needs --batch")
    if args.voxel and not args.ply:
        parser.error("--voxel needs --ply")
    if args.voxel and not (np.isfinite(args.voxel) and args.voxel > 0):
        parser.error("--voxel must be a length > 0")
    if args.top_view and not args.batch:
        parser.error("--top-view needs --batch")
    if args.ply and not args.batch:
        parser.error("--ply needs --batch")
    if args.occupancy and not args.batch:
        parser.error("--occupancy needs --batch")
    if args.batch < 0:
        parser.error("--batch must be >= 1")
    if args.batch and args.subsampling:
        parser.error("--batch does not take --subsampling (the per-frame path's zero-padded full-size map is not reproduced)")

    root = os.path.expanduser(args.kitti)
    if args.dataset == "kitti2015":
        ldir, rdir = os.path.join(root, "testing", "image_2"), os.path.join(root, "testing", "image_3")
    else:
        ldir, rdir = os.path.join(root, "image_02"), os.path.join(root, "image_03")
        if os.path.isdir(os.path.join(ldir, "data")):
            ldir, rdir = os.path.join(ldir, "data"), os.path.join(rdir, "data")
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ldir, "*.png")))
    if not files:
        parser.error("no PNG images under %s" % ldir)
    if args.frames:
        files = files[:args.frames]
    if args.out:
        os.makedirs(args.out, exist_ok=True)
    if args.top_view:
        os.makedirs(args.top_view, exist_ok=True)
    if args.ply:
        os.makedirs(args.ply, exist_ok=True)
    if args.occupancy:
        os.makedirs(args.occupancy, exist_ok=True)
    if args.voxel_render_spec is not None:
        os.makedirs(args.voxel_render_spec[0], exist_ok=True)
    if args.temporal_spec is not None:
        os.makedirs(args.temporal_spec[0], exist_ok=True)
    if args.odometry:
        _run_odometry(args, ldir, rdir, files)
    args.pose_rows = None
    if args.voxel_map:
        try:
            args.pose_rows = read_poses(args.poses, len(files))
            args.voxel_map_box = cli_voxel_map_box(args.pose_rows)
            voxel_map_params(args.voxel_map_box[0], args.voxel_map_box[1], args.voxel, CLI_VOXEL_MAP_CAPACITY)
        except (OSError, ValueError) as e:
            parser.error("--poses / --voxel-map: %s" % e)
        args.repose_rows = None
        if args.voxel_repose:
            try:
                args.repose_rows = read_poses12(args.voxel_repose, len(files))
                args.repose_box = cli_voxel_map_box(np.stack([args.repose_rows[:, 9], args.repose_rows[:, 10], np.arctan2(args.repose_rows[:, 3], args.repose_rows[:, 0])], 1))
                voxel_map_params(args.repose_box[0], args.repose_box[1], args.voxel, CLI_VOXEL_MAP_CAPACITY)
            except (OSError, ValueError) as e:
                parser.error("--voxel-repose: %s" % e)
    if args.occupancy_map:
        try:
            args.pose_rows = read_poses(args.poses, len(files))
            args.map_ranges = occupancy_map_cover(args.pose_rows, CLI_TOP_VIEW["x_range"], CLI_TOP_VIEW["y_range"])
            occupancy_map_params(args.map_ranges[0], args.map_ranges[1], CLI_TOP_VIEW["scale"])
        except (OSError, ValueError) as e:
            parser.error("--poses: %s" % e)
    if args.batch:
        _run_batched(args, ldir, rdir, files)
        return
    s = stereo_vision(width=1242 // args.scale, height=375 // args.scale, objectTracking=args.object_track, display=False, graphics=False,
                      scale=args.scale, pc_extrapolation=int(args.pointcloud_interpolation), CAMERA_CALIBRATION_YAML=args.camera_calibration,
                      subsampling=bool(args.subsampling))
    if args.rectify:
        s.sv.sv_legacy_set_rectify.argtypes = [ctypes.c_int]
        s.sv.sv_legacy_set_rectify.restype = None
        s.sv.sv_legacy_set_rectify(1)
    import time
    n = 0
    for name in files:
        left, right = _imread_bgr(os.path.join(ldir, name), args.scale), _imread_bgr(os.path.join(rdir, name), args.scale)
        if args.swap:
            left, right = right, left
        t0 = time.perf_counter()
        pts = s.generatePointCloud(left, right)
        dt = time.perf_counter() - t0
        print("(FPS=%f) (%d, %d) (t_t=%f) valid=%.3f" % (1.0 / dt, s.height, s.width, dt, float(np.isfinite(pts[:, 2]).mean())))
        if args.out:
            _write_png(os.path.join(args.out, name), s.last_disparity_u8())
        n += 1
    s.close()


def read_poses(path, n):
    """float64 [n, 3] = (x, y, yaw) from a text file with one such line per frame; ValueError unless it holds exactly n lines of three
    finite numbers (blank lines and lines that start with # do not count)."""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            words = line.split()
            if len(words) != 3:
                raise ValueError("a line of %s has %d words, not 'x y yaw'" % (path, len(words)))
            rows.append([float(w) for w in words])
    if len(rows) != n:
        raise ValueError("%s holds %d poses for %d frames" % (path, len(rows), n))
    out = np.array(rows, np.float64).reshape(n, 3)
    if not np.isfinite(out).all():
        raise ValueError("%s holds a pose that is not finite" % path)
    return out


def read_poses12(path, n):
    """float64 [n, 12] poses (R row-major, then t) from a text file with one line per frame, all of one form: 'x y yaw' as read_poses
    takes them, expanded by voxel_map_pose, or twelve words as --pose-graph writes them.  ValueError as read_poses, and for a file
    whose lines differ in form."""
    rows = []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                rows.append(line.split())
    if not rows or len(rows[0]) != 12:
        xyyaw = read_poses(path, n)
        return voxel_map_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2])
    if any(len(r) != 12 for r in rows):
        raise ValueError("a line of %s has not the twelve words of the first" % path)
    if len(rows) != n:
        raise ValueError("%s holds %d poses for %d frames" % (path, len(rows), n))
    out = np.array([[float(w) for w in r] for r in rows], np.float64).reshape(n, 12)
    if not np.isfinite(out).all():
        raise ValueError("%s holds a pose that is not finite" % path)
    return out


def cli_pose_graph_spec(text):
    """--pose-graph OUT[,ROUNDS[,GATE]] -> (OUT, rounds, gate or None); ValueError for an empty OUT, ROUNDS outside 1 .. 1000, a GATE
    that is negative or not finite, or more than three parts."""
    parts = text.split(",")
    if not parts[0] or len(parts) > 3:
        raise ValueError("OUT[,ROUNDS[,GATE]], got %r" % text)
    try:
        rounds, gate = int(parts[1]) if len(parts) > 1 else 10, float(parts[2]) if len(parts) > 2 else None
    except ValueError:
        raise ValueError("ROUNDS must be an integer and GATE a number, got %r" % text)
    if not 1 <= rounds <= 1000 or (gate is not None and not (gate >= 0.0 and np.isfinite(gate))):
        raise ValueError("ROUNDS in 1 .. 1000 and GATE finite and >= 0, got %r" % text)
    return parts[0], rounds, gate


CLI_POSE_GRAPH = dict(odometry=(1.0e4, 100.0),  # (w_rot, w_trans) of a step of the chain: 10 mrad and 0.1 m
                      refined=(1.0e4, 100.0),   # of a loop whose two poses the map's localisation refined: the same
                      coarse=(100.0, 1.0))      # of a loop known from the descriptor alone: a sector and a metre


def cli_pose_graph(path, xyyaw, went, found, sectors, refined, rounds=10, gate=None, device="cuda"):
    """--pose-graph's work: the chain of the run's poses xyyaw [N,3], a loop edge per (frame, key, shift) of `found` with frame != key -
    Z = went[key]^-1 o went[frame] where `refined` (went [N,12]: the poses the frames were inserted at), else went[key]^-1 o (the key's
    place under the recognised heading, place_guess) -, optimised by rig.PoseGraph on `device`, written to `path` twelve words a line by
    repr.  -> the corrected poses [N,12], the stats of pose_graph_optimize, the loop edges as (key, frame, Z)."""
    from ..rig import PoseGraph
    went = _poses_12(went, "went")
    g = PoseGraph(device=device)
    g.add_chain(voxel_map_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2]), *CLI_POSE_GRAPH["odometry"])
    loops = []
    for frame, key, shift in found:
        if frame == key:
            continue
        if refined:
            there = went[frame]
        else:
            at = place_guess(went[key:key + 1], np.array([shift]), sectors)[0]
            there = voxel_map_pose(at[0], at[1], at[3], at[2])
        Z = pose_between(went[key], there)
        g.add_loop(key, frame, Z, *CLI_POSE_GRAPH["refined" if refined else "coarse"])
        loops.append((key, frame, Z))
    poses, stats = g.optimize(rounds=rounds, gate=gate)
    with open(path, "w") as f:
        f.write("".join(" ".join("%r" % float(v) for v in row) + "\n" for row in poses))
    return poses, stats, loops


def occupancy_map_cover(poses_xyyaw, x_range, y_range):
    """(x_range, y_range), integers: the bounding box of a trajectory's (x, y) widened by the reach of a frame's grid - the largest
    distance of a corner of x_range x y_range from the vehicle, rounded up - so that every frame's grid falls into the map under any yaw."""
    reach = int(np.ceil(max(np.hypot(float(x), float(y)) for x in x_range for y in y_range)))
    p = np.asarray(poses_xyyaw, np.float64)
    return ((int(np.floor(p[:, 0].min())) - reach, int(np.ceil(p[:, 0].max())) + reach),
            (int(np.floor(p[:, 1].min())) - reach, int(np.ceil(p[:, 1].max())) + reach))


CLI_VOXEL_MAP_CAPACITY = 1 << 22  # voxels of --voxel-map's map: a table of 2^23 entries, 738 MB


def cli_voxel_map_box(poses_xyyaw):
    """(lo, hi) of --voxel-map's map: occupancy_map_cover of the trajectory in x and y, the CLI crop's z range."""
    (x0, x1), (y0, y1) = occupancy_map_cover(poses_xyyaw, CLI_TOP_VIEW["x_range"], CLI_TOP_VIEW["y_range"])
    return (float(x0), float(y0), CLI_CLOUD_CROP[0][2]), (float(x1), float(y1), CLI_CLOUD_CROP[1][2])


def cli_voxel_window_left(params, x, y):
    """--voxel-window's test: has the point (x, y) left the middle third of the box of `params` on the x or the y axis?"""
    for a, p in enumerate((x, y)):
        lo, hi = params["lo"][a], params["hi"][a]
        if not lo + (hi - lo) / 3.0 <= p <= hi - (hi - lo) / 3.0:
            return True
    return False


def cli_voxel_carry_text(stats):
    """The counts of a carry (a dict, or the int64 [4] tensor of the device) as the CLI prints them; reads a tensor back."""
    values = [stats[k] for k in VOXEL_CARRY_STATS] if isinstance(stats, dict) else [int(v) for v in stats.cpu().numpy()]
    return ", ".join("%s %d" % (k, v) for k, v in zip(VOXEL_CARRY_STATS, values))


def cli_voxel_align_spec(text):
    """(rounds, max_dist in cells, dof, method) of --voxel-align ROUNDS[,MAX_DIST_CELLS[,DOF[,point|plane]]]; ValueError for what
    voxel_map_align refuses."""
    words = text.split(",")
    if not 1 <= len(words) <= 4:
        raise ValueError("%d words, not ROUNDS[,MAX_DIST_CELLS[,DOF[,point|plane]]]" % len(words))
    rounds, max_dist, dof = int(words[0]), float(words[1]) if len(words) > 1 else 1.0, int(words[2]) if len(words) > 2 else 6
    method = words[3] if len(words) > 3 else "point"
    if rounds < 1 or dof not in (4, 6) or method not in VOXEL_ALIGN_METHODS:
        raise ValueError("ROUNDS >= 1, DOF 4 or 6 and point or plane, got %r" % (text,))
    voxel_align_max_d2(max_dist)
    return rounds, max_dist, dof, method


def cli_voxel_carve_spec(reach_m, min_miss, ratio, size):
    """(reach_m, min_miss, ratio) of --voxel-carve, checked as rig.VoxelMap.carve and voxel_map_carve check them: ValueError with the
    text the CLI prints."""
    if not (np.isfinite(reach_m) and reach_m > 0 and size > 0 and np.ceil(np.float64(reach_m) / np.float64(size)) <= VOXEL_CARVE_REACH_MAX):
        raise ValueError("REACH_M must be > 0 and at most %d cells of %g m, got %r" % (VOXEL_CARVE_REACH_MAX, size, reach_m))
    if min_miss < 1 or not 0 <= ratio <= 65535:
        raise ValueError("MIN_MISS >= 1 and RATIO in 0 .. 65535, got %d and %d" % (min_miss, ratio))
    return float(reach_m), int(min_miss), int(ratio)


def cli_voxel_carve_text(res):
    """The counts of a carve (the definition's dict, or the device's result with its int64 [4] stats) as the CLI prints them; reads a
    tensor back."""
    values = [res[k] for k in VOXEL_CARVE_STATS] if isinstance(res, dict) else [int(v) for v in res.stats.cpu().numpy()]
    return ", ".join("%s %d" % (k, v) for k, v in zip(VOXEL_CARVE_STATS, values))


def cli_voxel_render_spec(text):
    """(DIR, TOL_PX) of --voxel-render's DIR[,TOL_PX]: ValueError with the text the CLI prints."""
    words = text.rsplit(",", 1)
    try:
        tol = float(words[1]) if len(words) > 1 else 1.0
    except ValueError:
        raise ValueError("TOL_PX must be a number, got %r" % (words[1],))
    if not words[0] or not (np.isfinite(tol) and tol >= 0):
        raise ValueError("DIR[,TOL_PX] with TOL_PX >= 0, got %r" % (text,))
    return words[0], tol


def cli_voxel_flatten_spec(text, size):
    """((x0, x1), (y0, y1), scale, step_m, height_m) of --voxel-flatten's X0,X1,Y0,Y1,SCALE[,STEP_M[,HEIGHT_M]] for voxels of `size` metres,
    after occupancy_map_params' and voxel_flatten_params' checks: ValueError with the text the CLI prints."""
    words = text.split(",")
    if not 5 <= len(words) <= 7:
        raise ValueError("X0,X1,Y0,Y1,SCALE[,STEP_M[,HEIGHT_M]], got %r" % (text,))
    try:
        x0, x1, y0, y1, scale = (int(w) for w in words[:5])
        step, height = [float(w) for w in words[5:]] + [0.2, 2.0][len(words) - 5:]
    except ValueError:
        raise ValueError("X0, X1, Y0, Y1 and SCALE must be whole numbers, STEP_M and HEIGHT_M numbers, got %r" % (text,))
    flat = occupancy_map_params((x0, x1), (y0, y1), scale)
    if flat["rows"] * flat["cols"] > VOXEL_FLATTEN_CELLS_MAX:
        raise ValueError("a flat map of %d x %d cells: at most 8 000 000" % (flat["rows"], flat["cols"]))
    voxel_flatten_params(dict(lo=(0.0, 0.0, 0.0), size=size), None, step, height)
    return (x0, x1), (y0, y1), scale, step, height


def cli_voxel_flatten_text(stats):
    """voxel_map_flatten's eight counts as the CLI prints them."""
    return ", ".join("%s %d" % (k.replace("_", " "), int(v)) for k, v in zip(VOXEL_FLATTEN_STATS, stats))


CLI_VOXEL_CLUSTERS_ROWS = 65535  # rows of --voxel-clusters


def cli_voxel_clusters_spec(text, size):
    """(min_voxels, connectivity, h_lo_m, h_hi_m) of --voxel-clusters' MIN_VOXELS[,CONNECTIVITY[,H_LO_M,H_HI_M]] for voxels of `size`
    metres - the band None, None where it is not given -, after voxel_cluster_params' checks: ValueError with the text the CLI prints."""
    words = text.split(",")
    if len(words) not in (1, 2, 4):
        raise ValueError("MIN_VOXELS[,CONNECTIVITY[,H_LO_M,H_HI_M]], got %r" % (text,))
    try:
        min_voxels, connectivity = int(words[0]), int(words[1]) if len(words) > 1 else 26
        h_lo, h_hi = (float(words[2]), float(words[3])) if len(words) == 4 else (None, None)
    except ValueError:
        raise ValueError("MIN_VOXELS and CONNECTIVITY must be whole numbers, H_LO_M and H_HI_M numbers, got %r" % (text,))
    voxel_cluster_params(dict(lo=(0.0, 0.0, 0.0), size=size), connectivity, min_voxels, CLI_VOXEL_CLUSTERS_ROWS, 0, None, h_lo, h_hi)
    return min_voxels, connectivity, h_lo, h_hi


def cli_voxel_cluster_lines(boxes):
    """voxel_cluster_boxes' dict as the lines of <FILE>.clusters.txt: least key, voxels, the centre, the box's two corners, first and last
    frame."""
    return ["%d %d %s %d %d" % (key, voxels, " ".join(repr(float(v)) for v in list(c) + list(a) + list(b)), first, last)
            for key, voxels, c, a, b, first, last in zip(boxes["key"], boxes["voxels"], boxes["centre"], boxes["lo"], boxes["hi"], boxes["first_seq"], boxes["last_seq"])]


def voxel_cluster_colors(label):
    """uint8 [V,4] BGRA per voxel from its cluster's row (int [V], >= 0): a fixed hash of the row, never black."""
    lab = np.asarray(label, np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = lab * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x7F4A7C15)
    rgb = np.stack([(h >> np.uint64(s)) & np.uint64(0xFF) for s in (40, 48, 56)], -1).astype(np.int64)
    return np.concatenate([64 + rgb * 3 // 4, np.full((len(lab), 1), 255)], -1).astype(np.uint8)


def cli_voxel_render_text(counts):
    """The pixels per label of one view (six integers) as the CLI prints them."""
    return ", ".join("%s %d" % (k, int(v)) for k, v in zip(VOXEL_RENDER_LABELS, counts))


CLI_PLACE = dict(r_max=40.0, z_lo=-1.4, z_hi=1.0)  # --places: the reach and the heights of CLI_CLOUD_CROP, 20 rings of 60 sectors


def cli_places_spec(text):
    """--places FILE[,MIN_GAP[,ACCEPT]] -> (FILE, min_gap, accept); ValueError for an empty FILE, a MIN_GAP < 0, an ACCEPT outside 0 ..
    2^20 or more than three parts."""
    parts = text.split(",")
    if not parts[0] or len(parts) > 3:
        raise ValueError("FILE[,MIN_GAP[,ACCEPT]], got %r" % text)
    try:
        min_gap, accept = int(parts[1]) if len(parts) > 1 else 50, int(parts[2]) if len(parts) > 2 else 64
    except ValueError:
        raise ValueError("MIN_GAP and ACCEPT must be integers, got %r" % text)
    if not 0 <= min_gap <= 2 ** 31 - 1 or not 0 <= accept <= PLACE_ACCEPT_MAX:
        raise ValueError("MIN_GAP >= 0 and ACCEPT in 0 .. 2^20, got %r" % text)
    return parts[0], min_gap, accept


def cli_temporal_spec(text):
    """--temporal DIR[,TOL_PX[,MODE]] -> (DIR, tol_q in 1/16 px, mode); ValueError for an empty DIR, a TOL_PX outside 0 .. 65536, a MODE
    that is not fill, confirm or reject, or more than three parts."""
    parts = text.split(",")
    if not parts[0] or len(parts) > 3:
        raise ValueError("DIR[,TOL_PX[,MODE]], got %r" % text)
    try:
        tol = float(parts[1]) if len(parts) > 1 else 1.0
    except ValueError:
        raise ValueError("TOL_PX must be a number, got %r" % parts[1])
    if not (np.isfinite(tol) and 0.0 <= tol * 16.0 <= WARP_TOL_MAX):
        raise ValueError("TOL_PX in 0 .. 65536, got %r" % tol)
    mode = parts[2] if len(parts) > 2 else "fill"
    return parts[0], warp_words(tol_q=int(np.floor(tol * 16.0 + 0.5)), mode=mode)["tol_q"], mode


def cli_temporal_text(counts):
    """The label counts of a batch (int [pairs,8], WARP_COUNTS) as the CLI prints them: the sums over its pairs."""
    total = np.asarray(counts, np.int64).reshape(-1, 8).sum(0)
    return ", ".join("%s %d" % (k, int(v)) for k, v in zip(WARP_COUNTS, total))


def _write_temporal(args, rig, left, right, rel, ok, first, frame0):
    """--temporal for one batch of --odometry: frames frame0 .. of the folder, whose motions `rel` the odometry has fitted (`ok`)."""
    from ..engine import disparity_to_u8
    folder, tol_q, mode = args.temporal_spec
    motions = np.array(rel, np.float64).reshape(-1, 12)
    motions[~np.asarray(ok, bool)] = np.nan  # a pair without a motion keeps its measured map
    got = rig.temporal(left, right, pixel_format="bgr", poses=motions, mode=mode, tol_q=tol_q)
    img = disparity_to_u8(got["d1"]).cpu().numpy()
    lab = got["label"].cpu().numpy()
    d0 = got["d1"][0].cpu().numpy()
    for k in range(0 if first else 1, img.shape[0]):
        change = lab[k - 1] if k > 0 else (_flow_dq(d0) > 0).astype(np.uint8)  # the folder's first frame: nothing is expected
        _write_png(os.path.join(folder, "%06d.change.png" % (frame0 + k)), VOXEL_RENDER_PNG[change])
        _write_png(os.path.join(folder, "%06d.temporal.png" % (frame0 + k)), img[k])
    print("temporal: frames %d .. %d: %s" % (frame0 + 1, frame0 + img.shape[0] - 1, cli_temporal_text(got["counts"].cpu().numpy())))


def _write_png(path, u8):
    from PIL import Image
    Image.fromarray(u8).save(path)


def _run_odometry(args, ldir, rdir, files):
    """--odometry FILE: the folder through StereoRig.odometry, --batch frames at a time and the frame before them, each batch's first pair
    under the motion of the pair before it; the chained poses to FILE, the motions to FILE.rel.txt."""
    import torch
    from ..rig import StereoRig
    rig = StereoRig(1242 // args.scale, 375 // args.scale, calibration=args.camera_calibration, rectify=args.rectify, scale=args.scale)
    rel, ok = [], []
    tracks, track_lines = ObjectTracks(), []
    try:
        for i in range(0, len(files), args.batch):
            names = files[max(i - 1, 0):i + args.batch]
            lr = [(_imread_bgr(os.path.join(ldir, f), args.scale), _imread_bgr(os.path.join(rdir, f), args.scale)) for f in names]
            if args.swap:
                lr = [(r, l) for l, r in lr]
            left = torch.from_numpy(np.stack([l for l, _ in lr])).cuda(rig.device)
            right = torch.from_numpy(np.stack([r for _, r in lr])).cuda(rig.device)
            first = rel[-1] if rel and ok[-1] else None
            got = rig.odometry(left, right, pixel_format="bgr", first=first)
            if args.tracks and len(names) > 1:  # the same odometry once more, with the boxes: the batch's first frame is the last one's last
                tracked = rig.track(left, right, pixel_format="bgr", first=first)
                for frame, rows in tracks.feed({k: v.cpu().numpy() if hasattr(v, "cpu") else v for k, v in tracked.items() if k != "matches"}):
                    track_lines += tracks.lines(frame, rows)
            rel.extend(got["rel"])
            ok.extend(got["ok"])
            if args.temporal_spec is not None and len(names) > 1:
                _write_temporal(args, rig, left, right, got["rel"], got["ok"], i == 0, max(i - 1, 0))
    finally:
        rig.close()
    poses = flow_chain(np.array(rel).reshape(-1, 12), None, CAMERA_TO_VEHICLE, None, np.array(ok, bool))
    with open(args.odometry, "w") as f:
        f.write("".join(line + "\n" for line in flow_pose_lines(poses)))
    with open(args.odometry + ".rel.txt", "w") as f:
        f.write("".join(" ".join(repr(float(v)) for v in row) + "\n" for row in rel))
    print("odometry: %d frames, %d of %d motions fitted, written to %s" % (len(files), int(np.sum(ok)), len(ok), args.odometry))
    if args.tracks:
        with open(args.tracks, "w") as f:
            f.write("".join(line + "\n" for line in track_lines))
        print("tracks: %d ids over %d frames, %d lines written to %s" % (tracks.next_id, tracks.frame + 1, len(track_lines), args.tracks))


def _run_batched(args, ldir, rdir, files):
    """--batch N: the folder through a StereoRig (the batched front end and engine) N pairs at a time."""
    import time
    import torch
    from ..engine import (compact_cloud_from_disparity, disparity_to_u8, ground_from_disparity, occupancy_from_disparity, split_clouds,
                          split_voxel_clouds, top_view_from_disparity, voxel_cloud_from_disparity)
    from ..rig import StereoRig
    rig = StereoRig(1242 // args.scale, 375 // args.scale, calibration=args.camera_calibration, rectify=args.rectify, scale=args.scale)
    world = rig.occupancy_map(args.map_ranges[0], args.map_ranges[1], CLI_TOP_VIEW["scale"]) if args.occupancy_map else None
    model = rig.voxel_map(args.voxel_map_box[0], args.voxel_map_box[1], args.voxel, CLI_VOXEL_MAP_CAPACITY) if args.voxel_map else None
    places, recognised = (rig.place_index(**CLI_PLACE) if args.places_spec is not None else None), []
    n, busy, refined, refined_3d, aligned_3d = 0, 0.0, [], [], []
    try:
        for i in range(0, len(files), args.batch):
            names = files[i:i + args.batch]
            lr = [(_imread_bgr(os.path.join(ldir, f), args.scale), _imread_bgr(os.path.join(rdir, f), args.scale)) for f in names]
            if args.swap:
                lr = [(r, l) for l, r in lr]
            left = torch.from_numpy(np.stack([l for l, _ in lr])).cuda(rig.device)
            right = torch.from_numpy(np.stack([r for _, r in lr])).cuda(rig.device)
            torch.cuda.synchronize(rig.device)
            t0 = time.perf_counter()
            seen = None
            if args.ply:  # what rig.compact_clouds(..., transform=(CAMERA_TO_VEHICLE, None), lo=, hi=) runs, keeping d1 for the other outputs
                gl, gr, col = rig.frontend(left, right, pixel_format="bgr", colors=True)
                d1, _ = rig.engine.process_device(gl, gr, want_d2=False)
                if args.voxel:  # what rig.voxel_clouds(..., args.voxel, lo, hi, transform=(CAMERA_TO_VEHICLE, None)) runs
                    voxels = voxel_cloud_from_disparity(d1, rig.Q, args.voxel, CLI_CLOUD_CROP[0], CLI_CLOUD_CROP[1], colors=col, XR=CAMERA_TO_VEHICLE)
                    if model is not None:  # a frame that overflowed (count -1) adds nothing here and stops the run below, at split_voxel_clouds
                        at = args.pose_rows[i:i + len(names)]
                        if args.voxel_window and cli_voxel_window_left(model.params, at[0, 0], at[0, 1]):
                            print("voxel map recentred at frame %d: %s" % (i, cli_voxel_carry_text(model.recenter(at[0, 0], at[0, 1]))))
                        went = voxel_map_pose(at[:, 0], at[:, 1], at[:, 2])  # the poses the batch's frames are inserted at
                        if args.voxel_render_spec is not None:  # the map of the frames before this batch, seen from this batch's poses
                            seen = model.render(went, rig.render_camera(args.voxel), transform=(CAMERA_TO_VEHICLE, None), measured=d1, tol=args.voxel_render_spec[1])
                        if args.voxel_match_window is None:
                            if args.voxel_align_spec is not None and model.seq > 0:  # the whole batch against the frames before it
                                went = model.align(voxels[0], voxels[3], voxels[5], went, args.voxel_align_spec[0], args.voxel_align_spec[1], args.voxel_align_spec[2], method=args.voxel_align_spec[3])[0]
                            model.update(voxels[0], voxels[1], voxels[3], voxels[5], went)
                        for k in range(len(names) if args.voxel_match_window is not None else 0):  # one at a time: against the frames before it
                            one = [t[k:k + 1] for t in (voxels[0], voxels[1], voxels[3], voxels[5])]
                            guess = np.array([at[k, 0], at[k, 1], 0.0, at[k, 2]])
                            to = guess if model.seq == 0 else model.localize(one[0], one[2], one[3], guess, *args.voxel_match_window)[0][0]
                            refined_3d.append(to)
                            went[k] = voxel_map_pose(to[0], to[1], to[3], to[2])
                            if args.voxel_align_spec is not None and model.seq > 0:
                                went[k] = model.align(one[0], one[2], one[3], went[k:k + 1], args.voxel_align_spec[0], args.voxel_align_spec[1], args.voxel_align_spec[2], method=args.voxel_align_spec[3])[0][0]
                            model.update(*one, went[k:k + 1])
                        aligned_3d.extend(went)
                        if places is not None:  # a frame at a time: stored, then searched among the frames at least MIN_GAP before it
                            found = places.descriptor(voxels[0], voxels[3], voxels[5])
                            for k in range(len(names)):
                                one = {f: t[k:k + 1] for f, t in found.items()}
                                places.add(one, i + k, np.asarray(went[k:k + 1]))
                                recognised.append(places.query(one, i + k, args.places_spec[1], accept=args.places_spec[2])["best"])
                        if args.voxel_carve_spec is not None:  # the camera's centre is the origin of the vehicle axes: CAMERA_TO_VEHICLE only turns
                            reach_m, min_miss, ratio = args.voxel_carve_spec
                            res = model.carve(voxels[0], voxels[3], voxels[5], went, reach_m=reach_m, min_miss=min_miss, ratio=ratio)
                            print("voxel map carved after frame %d: %s" % (model.seq - 1, cli_voxel_carve_text(res)))
                    if model is not None and args.voxel_forget:
                        print("voxel map pruned after frame %d: %s" % (model.seq - 1, cli_voxel_carry_text(model.prune(since=model.seq - args.voxel_forget))))
                else:
                    clouds = compact_cloud_from_disparity(d1, rig.Q, colors=col, XR=CAMERA_TO_VEHICLE, lo=CLI_CLOUD_CROP[0], hi=CLI_CLOUD_CROP[1])
            else:
                d1 = rig.disparity(left, right, pixel_format="bgr")
            dmap = disparity_to_u8(d1)
            if args.top_view:  # what rig.top_view(..., disparity="d1", transform=(CAMERA_TO_VEHICLE, None)) gives, on the same d1
                grids = top_view_from_disparity(d1, rig.Q, XR=CAMERA_TO_VEHICLE, disparity="d1", **CLI_TOP_VIEW)
            if args.occupancy or world is not None:  # what rig.occupancy(..., transform=(CAMERA_TO_VEHICLE, None), **CLI_TOP_VIEW) gives, on the same d1
                g = ground_from_disparity(d1, rig.params.disp_max, want_vdisp=False)
                occ = occupancy_from_disparity(d1, g.labels, g.free_row, g.free_disp, rig.Q, XR=CAMERA_TO_VEHICLE, **CLI_TOP_VIEW)
            if world is not None:
                xyyaw = args.pose_rows[i:i + len(names)]
                if args.match_window is None:
                    world.update(occ, occupancy_pose(xyyaw[:, 0], xyyaw[:, 1], xyyaw[:, 2]))
                for k in range(len(names) if args.match_window is not None else 0):  # one at a time: a frame is matched against the frames before it
                    at = xyyaw[k] if world.seq == 0 else world.localize(occ.state[k:k + 1], xyyaw[k], *args.match_window, frame_grid=occ.spec)[0][0]
                    refined.append(at)
                    world.update(occ.state[k:k + 1], occupancy_pose(at[0], at[1], at[2])[None], occ.spec)
            torch.cuda.synchronize(rig.device)
            busy += time.perf_counter() - t0
            dmap = dmap.cpu().numpy()
            for name, m in zip(names, dmap):
                if args.out:
                    _write_png(os.path.join(args.out, name), m)
            if args.top_view:
                for name, g in zip(names, grids.cpu().numpy()):
                    _write_png(os.path.join(args.top_view, name), g)
            if args.occupancy:
                for name, st in zip(names, occ.state.cpu().numpy()):
                    _write_png(os.path.join(args.occupancy, name), OCCUPANCY_PNG[st])
            if seen is not None:  # BGRA to RGB; the labels through the palette
                for k, (bgra, lab, cnt) in enumerate(zip(seen.color.cpu().numpy(), seen.label.cpu().numpy(), seen.counts.cpu().numpy())):
                    _write_png(os.path.join(args.voxel_render_spec[0], "%06d.expected.png" % (i + k)), np.ascontiguousarray(bgra[..., 2::-1]))
                    _write_png(os.path.join(args.voxel_render_spec[0], "%06d.change.png" % (i + k)), VOXEL_RENDER_PNG[lab])
                    print("voxel map rendered before frame %d: %s" % (i + k, cli_voxel_render_text(cnt)))
            if args.ply:
                parts = split_voxel_clouds(voxels[0], voxels[5], voxels[1]) if args.voxel else split_clouds(clouds[0], clouds[3], clouds[1])
                for name, (xyz, color) in zip(names, parts):
                    write_ply(os.path.join(args.ply, os.path.splitext(name)[0] + ".ply"), xyz.cpu().numpy(), color.cpu().numpy())
            n += len(names)
            print("batch of %d (%d, %d): %.1f pairs/s so far" % (len(names), rig.height, rig.width, n / busy))
        if model is not None:
            print("voxel map: %d voxels of %g m written to %s" % (model.write_ply(args.voxel_map), args.voxel, args.voxel_map))
            if places is not None:
                lines = place_lines(range(len(recognised)), torch.cat(recognised).cpu().numpy(), places.params["sectors"]) if recognised else []
                with open(args.places_spec[0], "w") as f:
                    f.write("".join(line + "\n" for line in lines))
                print("places: %d of %d frames recognised an earlier one, written to %s" % (len(lines), len(recognised), args.places_spec[0]))
                if args.pose_graph_spec is not None:
                    best = torch.cat(recognised).cpu().numpy() if recognised else np.zeros((0, 4), np.int32)
                    found = [(f, int(b[0]), int(b[1])) for f, b in enumerate(best) if b[0] >= 0]
                    refined = args.voxel_match_window is not None or args.voxel_align_spec is not None
                    _, stats, loops = cli_pose_graph(args.pose_graph_spec[0], args.pose_rows, np.asarray(aligned_3d, np.float64).reshape(-1, 12), found,
                                                     places.params["sectors"], refined, args.pose_graph_spec[1], args.pose_graph_spec[2], device=rig.device)
                    print("pose graph: %d frames, %d loop edges (%d switched off), %d rounds, cost %r -> %r, written to %s" % (
                        len(args.pose_rows), len(loops), len(stats["off"]), stats["rounds"], stats["costs"][0] if stats["costs"] else stats["cost"], stats["cost"],
                        args.pose_graph_spec[0]))
            if args.voxel_match_window is not None:
                with open(os.path.splitext(args.voxel_map)[0] + ".poses.txt", "w") as f:
                    f.write("".join("%r %r %r %r\n" % tuple(float(v) for v in to) for to in refined_3d))
            if args.voxel_align_spec is not None:
                with open(os.path.splitext(args.voxel_map)[0] + ".aligned.txt", "w") as f:
                    f.write("".join(" ".join("%r" % float(v) for v in to) + "\n" for to in aligned_3d))
            if args.repose_rows is not None:  # from where the frames went to where the corrected poses put them; the stages below read the re-posed map
                fixed = args.repose_rows
                box = voxel_map_params(args.repose_box[0], args.repose_box[1], args.voxel, CLI_VOXEL_MAP_CAPACITY)
                text = cli_voxel_carry_text(model.repose(pose_corrections(np.asarray(aligned_3d, np.float64).reshape(-1, 12), fixed), params=box))
                out = os.path.splitext(args.voxel_map)[0] + ".reposed.ply"
                print("voxel map re-posed: %s; %d voxels written to %s" % (text, model.write_ply(out), out))
            if args.voxel_flatten_spec is not None:  # the planner's map from the voxel map's evidence
                x_range, y_range, scale, step, height = args.voxel_flatten_spec
                stem = os.path.splitext(args.voxel_map)[0] + ".flat"
                flat = rig.occupancy_map(x_range, y_range, scale)
                res = flat.load_voxels(model, step=step, height=height)
                np.savez(stem + ".npz", **dict({k: getattr(res, k).cpu().numpy() for k in ("logodds", "last_seen", "floor", "top")}, **{"map_" + k: v for k, v in flat.words.items()}))
                print("voxel map flattened into %d x %d cells, written to %s: %s" % (flat.words["rows"], flat.words["cols"], stem + ".npz", cli_voxel_flatten_text(res.stats.cpu().numpy())))
                if args.clearance and np.ceil(args.clearance * scale) <= CLEARANCE_RADIUS_MAX:
                    _write_png(stem + ".clearance.png", clearance_png(flat.clearance(args.clearance).cpu().numpy()))
                    if args.goal_xy is not None:
                        field = flat.cost_to_goal(args.goal_xy, args.clearance)
                        route, xy = flat.routes(refined[-1][:2] if refined else args.pose_rows[-1, :2])
                        length = int(route.length[0])
                        with open(stem + ".route.txt", "w") as f:
                            f.write("".join("%d %d %r %r\n" % (r, c, float(x), float(y)) for (r, c), (x, y) in zip(route.cells[0, :length].cpu().numpy(), xy[0, :length])))
                        print("route on the flattened map: status %d, %d cells%s" % (int(route.status[0]), length, "" if field.converged else " (field not converged)"))
            if args.voxel_clusters_spec is not None:  # the objects of the map; over the flat map's floor where one was made
                from ..engine import voxel_cluster_boxes, voxel_cluster_labels
                min_voxels, connectivity, h_lo, h_hi = args.voxel_clusters_spec
                over = {}
                if args.voxel_flatten_spec is not None:
                    over = dict(flat=flat, h_lo=args.voxel_flatten_spec[3] if h_lo is None else h_lo, h_hi=args.voxel_flatten_spec[4] if h_hi is None else h_hi)
                else:
                    over = dict(h_lo=h_lo, h_hi=h_hi)
                found = model.clusters(connectivity, min_voxels, CLI_VOXEL_CLUSTERS_ROWS, **over)
                stem = os.path.splitext(args.voxel_map)[0] + ".clusters"
                boxes = voxel_cluster_boxes(found, model.params)
                with open(stem + ".txt", "w") as f:
                    f.write("".join(line + "\n" for line in cli_voxel_cluster_lines(boxes)))
                key, lab = (t.cpu().numpy() for t in voxel_cluster_labels(found))
                rows = model.rows()
                at = np.searchsorted(key, rows["key"].cpu().numpy())  # every voxel of rows() holds a key of the table
                in_cluster = lab[at] >= 0
                write_ply(stem + ".ply", rows["xyz"].cpu().numpy()[in_cluster], voxel_cluster_colors(lab[at][in_cluster]))
                info = found.info.cpu().numpy()
                print("voxel map clustered: %d members, %d components, %d of at least %d voxels (the largest %d), written to %s and %s"
                      % (info[0], info[1], info[2], min_voxels, info[5], stem + ".txt", stem + ".ply"))
        if world is not None:
            _write_png(args.occupancy_map, OCCUPANCY_PNG[world.state().cpu().numpy()])
            if args.clearance:
                _write_png(os.path.splitext(args.occupancy_map)[0] + ".clearance.png", clearance_png(world.clearance(args.clearance).cpu().numpy()))
            field, last_xy = None, (refined[-1][:2] if refined else args.pose_rows[-1, :2])
            if args.goal_xy is not None:  # the field under the clearance just made, and the route from where the drive ended
                field = world.cost_to_goal(args.goal_xy, args.clearance)
            if args.frontiers:  # under the pen of a cost-to-goal field: the one just made, or one towards where the drive ended
                if field is None:
                    world.cost_to_goal(last_xy, args.clearance)
                found = world.frontiers(min_cells=args.frontiers)
                clusters = found.clusters.cpu().numpy()
                print("".join(line + "\n" for line in frontier_lines(world.words, clusters, found.info.cpu().numpy())), end="")
                _write_png(os.path.splitext(args.occupancy_map)[0] + ".frontiers.png", frontier_png(found.label.cpu().numpy(), clusters))
                goals = world.frontier_goals(found)
                if args.view_spec is not None:
                    fov, range_m, rays, headings = args.view_spec
                    arrive, seen = world.frontier_views(found, headings=headings, fov=fov, range_m=range_m, n_rays=rays)
                    print("".join(line + "\n" for line in view_lines(arrive, seen.counts.cpu().numpy(), seen.best.cpu().numpy(), seen.best_score.cpu().numpy())), end="")
                if field is None and len(goals):
                    field = world.cost_to_goal(goals, args.clearance)
            if field is not None:
                route, xy = world.routes(last_xy)
                length, status = int(route.length[0]), int(route.status[0])
                cells = route.cells[0, :length].cpu().numpy()
                with open(os.path.join(os.path.dirname(os.path.abspath(args.occupancy_map)), "route.txt"), "w") as f:
                    f.write("".join("%d %d %r %r\n" % (r, c, float(x), float(y)) for (r, c), (x, y) in zip(cells, xy[0, :length])))
                at_start = int(field.cost[int(cells[0, 0]), int(cells[0, 1])]) if length else None
                print("route: status %d, %d cells, cost at the start %s%s" % (status, length, at_start, "" if field.converged else " (field not converged)"))
        if args.match_window is not None:
            with open(os.path.splitext(args.occupancy_map)[0] + ".poses.txt", "w") as f:
                f.write("".join("%r %r %r\n" % tuple(float(v) for v in at) for at in refined))
    finally:
        rig.close()
    print("pairs/s %.1f (%d pairs, batch %d)" % (n / busy if busy else 0.0, n, args.batch))
