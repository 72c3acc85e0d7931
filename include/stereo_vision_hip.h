/*
 * libstereo_vision_hip.so — C ABI of the MI355X-native stereo disparity engine.
 *
 * Plain C: pointers and sizes only, no torch / C++ types.  Three groups of entry points:
 *
 *  (A) The reference's own exported symbols, kept signature-for-signature so that the reference's
 *      ctypes binding (stereo_vision/sv.py:164-192) drives this library unchanged:
 *        generatePointCloud   reference: src/serial_includes/main/stereo_vision.cpp:565-623
 *        clean                reference: src/serial_includes/main/stereo_vision.cpp:105-114
 *        getColor             reference: src/serial_includes/main/stereo_vision.cpp:625-627
 *
 *  (B) The operator seam the reference's driver calls once per frame,
 *        Elas::process(I1, I2, D1, D2, dims)   reference: src/serial_includes/elas/elas.h:162,
 *                                               called from stereo_vision.cpp:296-318
 *      exposed as a handle-based, batched API (sv_*): the reference keeps all state in file-scope
 *      globals and function statics (stereo_vision.cpp:50-89, 307-314, 582) and processes one pair
 *      per call; here state lives in an sv_handle and one call takes B independent pairs.
 *
 *  (C) The camera front end in front of (B): a calibrated rig (sv_rig_*) turns batches of colour or gray camera
 *      frames into the engine's input; the legacy entry (A) is one of its clients.
 *
 *  (D) Behind (B): bird's-eye views (sv_top_view_*) - 2-D ground grids of where a batch of point clouds, or of clouds
 *      reprojected from disparity maps on the fly, fell (the reference's points_2_top_view helper, stereo_vision/sv.py:87-134).
 *
 *  (E) Behind (B) as well: the 3-D position of each detected object (sv_box_positions_*) - the mean of the points inside a
 *      detector's boxes, for batches, from disparity maps (fused: no cloud is written) or from point clouds (publishPointCloud's
 *      per-object step, src/serial_includes/main/stereo_vision.cpp:261-278).
 *
 *  (F) Behind (B) as well: compact coloured point clouds (sv_cloud_*) - per pair the list of valid, cropped, thinned-out 3-D
 *      points with their colours and pixel indices, in pixel order, from disparity maps (fused: no dense cloud is written).  It is
 *      what the reference's viewer draws: Grapher pairs points[i] with colors[i] (src/common_includes/graphing.h:123-133).
 *
 *  (G) Behind (B) as well: the ground plane, obstacle labels and free space (sv_ground_*) - per pair the v-disparity histogram, the
 *      ground line fitted to it, a label per pixel and per column the base of the nearest obstacle, from disparity maps.  The reference
 *      has no counterpart; stereo_vision.sv states the definition in numpy.
 *
 *  (H) Behind (G): the stixel world and detector-free object boxes (sv_stixel_*) - per image column the vertical segments of obstacle
 *      pixels that stand at one disparity, and the groups of neighbouring columns whose nearest segments agree, as boxes in (E)'s layout.
 *      The reference takes its boxes from a detector; stereo_vision.sv states this definition in numpy.
 *
 *  (I) Behind (B) as well: voxel-grid downsampled clouds (sv_voxel_*) - per pair one row per occupied cell of a regular 3-D grid over
 *      (F)'s points: the centroid, the mean colour and the number of points, in the order a scan of the image meets the cells, from
 *      disparity maps (fused: neither a dense cloud nor the list of points is written).  stereo_vision.sv states the definition in numpy.
 *
 *  (K) Behind (J): a world-fixed occupancy map (sv_occupancy_map_spec, the fuse entry) - the per-frame grids of a drive fused along the poses
 *      of its odometry into one log-odds map that accumulates evidence, comes back down where a cell is seen free again, and scrolls
 *      with the vehicle.  stereo_vision.sv.occupancy_fuse states the definition in numpy.
 *
 *  (L) Behind (K): the correlative match (sv_map_match_*) - how well a frame's grid of (J) fits the map of (K) at each of a set of candidate
 *      poses, and the best of them, so that a drifting pose can be corrected before the frame is fused.  stereo_vision.sv.occupancy_match
 *      states the definition in numpy.
 *
 *  (M) Behind (K) as well: what a planner asks of the map (sv_clearance_*) - the capped exact squared distance from every cell to the
 *      nearest occupied (or never seen) cell, and a batched check of candidate paths' footprints against that field.
 *      stereo_vision.sv.occupancy_clearance and clearance_paths state the definitions in numpy.
 *
 *  (Q) Behind (I) and (F): a world-fixed voxel map (sv_voxel_map_*) - the voxel rows or the compact clouds of the frames of a drive, moved
 *      into the world by one pose per frame and accumulated per cubic cell in a table that persists from call to call: one coloured 3-D
 *      model of what the drive has seen.  stereo_vision.sv.voxel_map_insert and voxel_map_rows state the definition in numpy.
 *
 *  (R) Behind (Q): a frame matched against the voxel map (sv_voxel_match_*) - how well the rows of a frame fit the map of (Q) at each of a
 *      set of candidate 3-D poses, and the best of them, so that a pose - its height and its heading included - can be corrected before the
 *      frame is inserted.  stereo_vision.sv.voxel_map_match states the definition in numpy.
 *
 *  (S) Behind (R): a voxel map carried into another (sv_voxel_map_carry_device) - the voxels of a map of (Q), filtered and shifted by whole
 *      cells, added into a second map: a prune (same box, empty destination), a scroll (a shifted box), a grow (a larger capacity) or a
 *      merge (a destination that holds voxels), so that the map can follow the vehicle and forget.  stereo_vision.sv.voxel_map_carry
 *      states the definition in numpy.
 *
 *  (T) Behind (S): a voxel map carved by the sight lines of frames (sv_voxel_carve_device) - a ray per row of a frame from the sensor's cell
 *      through the table of (Q); a voxel that enough rays of later frames pass through is emptied, so that the map can un-see a car that
 *      drove away or a mismatch at a depth edge.  stereo_vision.sv.voxel_map_carve states the definition in numpy.
 *
 *  (U) Behind (T): the voxel map rendered into a camera (sv_voxel_render_device) - per view the nearest voxel of (Q)'s table under every
 *      pixel: its depth, key and colour, the disparity the rig would measure there, and a per-pixel comparison with the disparity it did
 *      measure, which names what is new and what was seen through.  stereo_vision.sv.voxel_map_render states the definition in numpy.
 *
 *  (V) Behind (T): the voxel map flattened into (K)'s layout (sv_voxel_flatten_device) - the voxels of (Q)'s table sliced by their height
 *      above an absolute or a local floor into ground, obstacle and overhead, and per flat cell the logodds and last_seen words that (M)
 *      to (P) take, so that the planner runs on the voxel map.  stereo_vision.sv.voxel_map_flatten states the definition in numpy.
 *
 *  (W) Behind (V): the voxel map clustered (sv_voxel_clusters_device) - the 6-, 18- or 26-connected components of the voxels of (Q)'s
 *      table inside a height band, over an absolute floor or over (V)'s: a row of counts, sums and a box per component, a label per slot,
 *      and the components below a size emptied - the objects of the map and its speckle filter.  stereo_vision.sv.voxel_map_clusters
 *      states the definition in numpy.
 *
 *  (X) Behind (R): a frame aligned to the voxel map (sv_voxel_align_*) - every row of a frame paired with the nearest voxel mean of (Q)'s
 *      table and the pairs reduced to the nineteen integers a closed-form rigid fit needs: one round of iterative closest point, so
 *      that a pose is refined below (R)'s step and in roll and pitch as well.  stereo_vision.sv.voxel_map_align_sums states the definition
 *      in numpy; voxel_align_solve and voxel_map_align are the fit and the loop around both.
 *
 *  (Y) Behind (X): the surface normals of the voxels (sv_voxel_normals_device) - per voxel of (Q)'s table a plane fitted to the means of
 *      the voxels around it, as the best of a fixed table of integer directions under an exact integer criterion - and the sums of one
 *      round of point-to-plane alignment against them (sv_voxel_plane_align_*): (X)'s pairs, each reduced along its partner's normal, so
 *      that a row may slide along the ground or a wall it lies on and the loop converges in a few rounds where (X)'s creeps.
 *      stereo_vision.sv.voxel_map_normals and voxel_map_align_plane_sums state the definitions in numpy; voxel_align_solve_plane is the fit.
 *
 *  (Z) Behind the engine, in front of every stage that takes a pose: stereo visual odometry (sv_flow_*) - the lattice points of frame k - 1
 *      that carry a disparity found again in frame k by a sum of absolute differences over a window around where a guessed motion puts
 *      them (sv_flow_match_device), and the matches reduced, under a pose, to the 32 integers of one gated Gauss-Newton round of the
 *      camera's motion between the two frames (sv_flow_pose_sums_device).  stereo_vision.sv.flow_match and flow_pose_sums state the
 *      definitions in numpy; flow_solve, flow_egomotion and flow_chain are the fit, the loop and the chain of poses on the host.
 *
 *  (AA) Behind the engine and (Z), in front of every stage that takes a disparity map: temporal consistency (sv_disparity_warp_*) - the
 *      map of frame k - 1 warped into frame k under the motion between them, the nearest source per pixel kept, and the prediction held
 *      against what frame k measured: a label per pixel (agree, nearer, farther, measured only, expected only) and a filtered map - gaps
 *      filled from the frame before, or only what it confirms, or all but what it contradicts.  stereo_vision.sv.disparity_warp states
 *      the definition in numpy.
 *
 *  (AB) Behind (Z), (H) and (E): object links (sv_object_links_*) - the temporal matches of (Z1) sorted into the boxes of frames k - 1 and
 *      k, a vote per pair of boxes, a link per previous box, and each linked box's matches reduced to the integers of its own motion, the
 *      motion that remains once the camera's is taken out.  stereo_vision.sv.object_links states the definition in numpy; object_motion
 *      and ObjectTracks are the metres and the bookkeeping of ids, velocities and predictions on the host.
 *
 *  (AC) Beside (Q) and behind (L): place recognition (sv_place_*) - a frame of rows reduced to a polar height image around the vehicle,
 *      rings x sectors bytes that a turn of the vehicle rolls along the sectors (AC1), and query descriptors searched among stored ones
 *      under every roll, the best key per query by the least sum of absolute differences over the sum of both descriptors (AC2).
 *      stereo_vision.sv.place_descriptor and place_match state the definitions in numpy; place_yaw and place_guess turn a key and a
 *      shift into the guess the voxel map's localisation takes.  The solver for the confirmed loops is (AE); its result goes to (AD).
 *
 *  (AD) Behind (AC), (S) and (Q): a voxel map re-posed after a loop closure (sv_voxel_repose_device) - every voxel of a map of (Q) moved
 *      by the rigid correction of the frame that saw it last, one of K corrections chosen by the voxel's last_seq, and accumulated into a
 *      second map with (Q)'s integer atomics: what the pose graph of (AE) returns - a corrected pose per frame - applied to a map whose
 *      frames are gone.  stereo_vision.sv.voxel_map_repose states the definition in numpy; pose_corrections turns the old and the new
 *      poses into the corrections, and loop_spread is the host's helper for one confirmed loop without a graph.
 *
 *  (AE) Between (AC) and (AD): the pose graph of confirmed loops (sv_pose_graph_*) - a pose per frame, odometry edges along the chain and
 *      loop edges across it, each a measured relative pose with two weights; one Gauss-Newton linearisation in doubles without
 *      trigonometry (AE1) and preconditioned conjugate gradients on it, matrix-free, with the state of the iteration on the device
 *      (AE2).  stereo_vision.sv.pose_graph_linearize, pose_graph_pcg and pose_graph_sum state the definitions in numpy;
 *      pose_graph_optimize is the loop of rounds on the host, with the gate that switches a wrong loop off.
 *
 * All sv_* functions return SV_OK (0) or a negative sv_status; sv_last_error() gives the text.
 * Nothing in this library calls exit().
 */
#ifndef STEREO_VISION_HIP_H
#define STEREO_VISION_HIP_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (B) batched Elas::process ------------------------------------------------------------------------ */

/* Field-for-field mirror of Elas::parameters (reference: src/serial_includes/elas/elas.h:60-145);
 * every bool is an int32 so the block is 23 four-byte words. */
typedef struct sv_params {
    int32_t disp_min;              /* elas.h:61  first disparity of the support matching's search (elas.cpp:318; negative = 0; both presets use 0) */
    int32_t disp_max;              /* elas.h:62  D = disp_max + 1, 10 <= disp_max <= 1023 */
    float support_threshold;       /* elas.h:63 */
    int32_t support_texture;       /* elas.h:64 */
    int32_t candidate_stepsize;    /* elas.h:65  >= 1; the support matching's LDS (160 KiB per workgroup) bounds it by disp_max: 32 (126 step + 3 disp_max + 22)
                                    * + 4352 bytes must fit, i.e. step <= 15 at disp_max 1023, <= 37 at 63 (the even step of half resolution counts) */
    int32_t incon_window_size;     /* elas.h:66 */
    int32_t incon_threshold;       /* elas.h:67 */
    int32_t incon_min_support;     /* elas.h:68 */
    int32_t add_corners;           /* elas.h:69 */
    int32_t grid_size;             /* elas.h:70 */
    float beta;                    /* elas.h:71 */
    float gamma;                   /* elas.h:72 */
    float sigma;                   /* elas.h:73 */
    float sradius;                 /* elas.h:74 */
    int32_t match_texture;         /* elas.h:75 */
    int32_t lr_threshold;          /* elas.h:76 */
    float speckle_sim_threshold;   /* elas.h:77 */
    int32_t speckle_size;          /* elas.h:78 */
    int32_t ipol_gap_width;        /* elas.h:79 */
    int32_t filter_median;         /* elas.h:80 */
    int32_t filter_adaptive_mean;  /* elas.h:81 */
    int32_t postprocess_only_left; /* elas.h:82 */
    int32_t subsampling;           /* elas.h:83  (bool) half-resolution mode: disparity maps are (width/2) x (height/2) */
} sv_params;

enum sv_setting { SV_ROBOTICS = 0, SV_MIDDLEBURY = 1, SV_DRIVER = 2 };

/* SV_ROBOTICS / SV_MIDDLEBURY: the two presets of elas.h:92-143.
 * SV_DRIVER: what the reference driver actually runs (stereo_vision.cpp:307-311):
 *            MIDDLEBURY + postprocess_only_left + filter_adaptive_mean. */
void sv_params_init(sv_params *p, int setting);

typedef enum sv_status {
    SV_OK = 0,
    SV_ERR_ARG = -1,         /* bad argument / unsupported parameter value */
    SV_ERR_HIP = -2,         /* a HIP runtime call failed */
    SV_ERR_NO_DEVICE = -3,   /* no usable GPU */
    SV_ERR_UNSUPPORTED = -4, /* a test hook's input beyond what its kernel takes */
    SV_ERR_STATE = -5
} sv_status;

typedef struct sv_handle sv_handle;

/* Engine configuration beyond the ELAS parameters.  Every field is an int32; 0 always means "the default" (zero-initialise the struct and
 * set what you need).  The policy fields below n_slots used to be environment variables; the variables are still read - in ONE place,
 * engine.cpp: apply_env_overrides - and override the fields, so that a deployment can be steered without a rebuild; two handles of
 * one process can be configured differently through the fields. */
typedef struct sv_config {
    int32_t width;      /* image width  (>= 32) */
    int32_t height;     /* image height (>= 32) */
    int32_t device;     /* HIP device ordinal */
    int32_t n_workers;  /* host pool threads for the CPU stage between the two GPU phases (0 = default: the cgroup CPU quota / the
                         * affinity mask, shared between the ranks of a node, at most 16 without a quota) */
    int32_t chunk;      /* pairs per GPU launch = pairs per pipeline slot (0 = default 64, less for large images) */
    int32_t keep_debug; /* != 0: keep per-stage intermediates of the LAST processed pair for sv_debug_get */
    int32_t n_streams;  /* HIP streams the second GPU phase alternates over (0 = default 5; 4 for images of 2 M pixels and more); phase 1 has its own streams */
    int32_t n_slots;    /* buffer slots (chunks in flight) of the 3-stage pipeline (0 = default 8, within a quarter of the free HBM / 64 GB) */
    /* ---- policy (0 = automatic) */
    int32_t gpu_lattice_filter;    /* support-lattice filters: 0 auto (GPU for chunk >= 4), 1 GPU, 2 host pool             [SV_GPU_FILTER=1 / SV_HOST_FILTER=1] */
    int32_t gpu_triangulation;     /* who triangulates: 0 auto (pool and GPU balanced by the pool's backlog; GPU alone with < 3 host threads),
                                      1 GPU, 2 host pool, 3 a fixed share of gpu_triangulation_pct percent on the GPU, 4 balanced by the pool's
                                      backlog whatever the number of host threads                                        [SV_GPU_DELAUNAY=1/0, SV_GPU_DELAUNAY_PCT=n, SV_GPU_DELAUNAY_AUTO=0] */
    int32_t gpu_triangulation_pct; /* the share for mode 3 (1..100) */
    int32_t resident;              /* the GPU's share without the support lists ever leaving the device: 0 auto (on), 2 off  [SV_RESIDENT=0] */
    int32_t dg_sub_max;            /* > 0: vertices a set may have to be triangulated whole in LDS (default 4000; experiments, tests) [SV_DG_SUBMAX] */
    int32_t dg_max_points;         /* > 0: largest vertex set the GPU kernels take, larger ones go to the pool (tests)       [SV_GPU_DELAUNAY_MAX] */
    int32_t affinity;              /* host threads on the CPUs of the GPU's NUMA node: 0 auto (when the node has enough allowed CPUs), 2 never [SV_NO_AFFINITY=1] */
    int32_t inline_latency_path;   /* single pairs on a chunk-1 handle driven by the calling thread: 0 auto (on), 2 off       [SV_NO_INLINE=1] */
    int32_t event_sync;            /* how host threads wait for the GPU: 0 auto (3 for chunk >= 4, 2 below), 1 hipEventBlockingSync, 2 spin, 3 ask the event + 40 us naps [SV_EVENT_SYNC=block|spin|poll] */
    int32_t share_sliced;          /* != 0: a balanced GPU share as a slice of every chunk instead of whole chunks (round-2 behaviour, non-resident only) [SV_GPU_DELAUNAY_SLICED=1] */
    int32_t latency_split;         /* single pairs: 0 automatic - each triangulation in quarters (seven helper cores) or halves (four) on pool threads pinned to
                                      cores that share the calling thread's L3 cache, when the host has such cores within the process's mask (and affinity != 2),
                                      otherwise as 3; 1 halves / 2 quarters of the top-level cuts on pool threads in any case; 3 each triangulation on one thread
                                      [SV_LATENCY_SPLIT=0..3] */
    int32_t host_copies;           /* host-memory batches (sv_submit_batch_host...): who moves images and maps over PCIe.  0 auto = 2 where the runtime
                                      allows it, 1 hipMemcpyAsync (the runtime picks an SDMA engine per copy - the directions can end up sharing
                                      one), 2 engine-addressed copies (csrc/dma_lanes.cpp): uploads and downloads on SDMA engines of their own,
                                      queued ahead of the kernels                                                          [SV_HOST_COPIES=1|2] */
    int32_t reserved[4];           /* must be 0 (sv_create checks) */
} sv_config;

int sv_create(const sv_params *params, const sv_config *cfg, sv_handle **out);
int sv_destroy(sv_handle *h);
/* What the handle decided at creation (defaults depend on the image size, the free memory and the CPU quota). */
enum sv_query_key {
    SV_Q_HOST_THREADS = 0,       /* size of the host pool */
    SV_Q_CHUNK = 1,              /* pairs per GPU launch */
    SV_Q_SLOTS = 2,              /* chunks in flight */
    SV_Q_GPU_LATTICE_FILTER = 3, /* 1: support-lattice filters on the GPU, 0: on the host pool */
    SV_Q_GPU_TRIANGULATION = 4,  /* 1: Delaunay divide-and-conquer on the GPU (few host threads), 0: on the host pool */
    SV_Q_GPU_TRIANGULATION_FALLBACKS = 6, /* vertex sets handed to the GPU kernel's share that the host triangulated after all (coincident points,
                                             whose survivor the reference's quicksort decides; more vertices than the kernels take) */
    SV_Q_NUMA_BOUND = 7,         /* 1: the handle's host threads are bound to the CPUs of the GPU's NUMA node (SV_NO_AFFINITY=1 disables) */
    SV_Q_RESIDENT = 8,           /* 1: the GPU's share of the chunks is built "resident" - the support lists never leave the device: sort, duplicate scan,
                                    k-d order and triangulation in one kernel after the lattice filter; the host only reads 8 meta words per pair */
    SV_Q_HOST_COPIES = 9,        /* who moves host-memory batches over PCIe: 0 not decided yet (no such batch so far), 1 hipMemcpyAsync,
                                    2 engine-addressed SDMA copies (sv_config.host_copies) */
    SV_Q_LATENCY_SPLIT = 10,     /* single pairs: 0 each triangulation on one thread, 1 in halves, 2 in quarters (sv_config.latency_split as resolved at creation) */
    SV_Q_GPU_TRIANGULATION_SHARE = 5 /* per mille of the pairs so far whose triangulations the GPU kernel built (in the host mode the
                                        dispatcher hands it a share of a chunk while the pool is behind; results are identical) */
};
int sv_query(const sv_handle *h, int what);
const char *sv_last_error(const sv_handle *h); /* h may be NULL: error of the last failed sv_create */

/* B independent pairs, images and maps in DEVICE memory (HBM):
 *   left/right : uint8  [B][height][stride]   rectified gray rows (what Elas::process receives as I1/I2)
 *   d1 / d2    : float  [B][height][width]    disparity maps (what Elas::process writes to D1/D2); with params.subsampling
 *                                             the maps are [B][height/2][width/2] (elas.h:160-161);
 *                                             d2 may be NULL.  Invalid pixels are -10 (elas.cpp:823-824, 987-991).
 *   status     : int32  [B] host array, may be NULL; per pair: number of support points, or <3 when the
 *                reference would have printed "ERROR: Need at least 3 support points!" (elas.cpp:63-69) — the
 *                maps of such a pair are left untouched, as the reference leaves them.
 * The call returns when all B pairs are complete (outputs visible to every stream of the device). */
int sv_process_batch_device(sv_handle *h, const uint8_t *left, const uint8_t *right, int batch, int stride, float *d1, float *d2, int32_t *status);

/* Streaming form: sv_submit_batch_device enqueues a batch and returns at once; batches are processed in submission order and
 * flow through the same pipeline back to back (the first chunks of batch k+1 overlap the last chunks of batch k).  sv_wait
 * returns when every submitted batch is complete.  Buffers must stay valid until then.  sv_process_batch_device == submit + wait. */
int sv_submit_batch_device(sv_handle *h, const uint8_t *left, const uint8_t *right, int batch, int stride, float *d1, float *d2, int32_t *status);
int sv_wait(sv_handle *h);
/* Returns when the n oldest batches submitted since the last sv_wait are complete; later ones keep running (batches complete in
 * submission order).  For consumers that take finished batches while the engine computes the next - e.g. a chunked gather of the
 * maps on one rank that overlaps the other chunks' kernels.  Not to be called concurrently with sv_wait. */
int sv_wait_batches(sv_handle *h, int n);

/* Same call with HOST memory in and out - the form of the reference's seam, which takes host pointers (elas.h:162, call site
 * stereo_vision.cpp:313).  The batch streams through the pipeline chunk by chunk: the images of chunk k+1 go up and the maps of
 * chunk k-1 come down on copy streams while chunk k computes; nothing is allocated per call.  Page-locked ("pinned") caller
 * memory - sv_host_alloc, hipHostMalloc, hipHostRegister, torch pin_memory() - is the DMA source / target itself; pageable
 * memory is detected and goes through page-locked staging buffers of the handle (one extra host copy each way).  Maps of pairs
 * with < 3 support points are not written (the reference leaves them untouched, elas.cpp:63-69).
 * sv_submit_batch_host is the streaming form (buffers stay valid and untouched until sv_wait). */
int sv_process_batch_host(sv_handle *h, const uint8_t *left, const uint8_t *right, int batch, int stride, float *d1, float *d2, int32_t *status);
int sv_submit_batch_host(sv_handle *h, const uint8_t *left, const uint8_t *right, int batch, int stride, float *d1, float *d2, int32_t *status);
/* The same with the DRIVER's output format: dmap = saturate(round_half_even(4 * D1)) as uint8 [B][height][width] (what the reference's
 * generateDisparityMap returns: leftdpf.convertTo(dmap, CV_8UC1, 4.0), stereo_vision.cpp:316; [B][height/2][width/2] with
 * params.subsampling), converted on the device: a quarter of the bytes come back over PCIe.  Images of pairs with < 3 support
 * points are not written.  Page-locked or pageable memory, like above. */
int sv_process_batch_host_dmap(sv_handle *h, const uint8_t *left, const uint8_t *right, int batch, int stride, uint8_t *dmap, int32_t *status);
int sv_submit_batch_host_dmap(sv_handle *h, const uint8_t *left, const uint8_t *right, int batch, int stride, uint8_t *dmap, int32_t *status);
/* Page-locked host memory for the calls above (NULL on failure). */
void *sv_host_alloc(size_t bytes);
void sv_host_free(void *p);

/* Single pair with the exact argument meaning of Elas::process (elas.h:153-162): dims = {width, height, bytes per line};
 * host pointers, like the reference.  On a chunk = 1 handle the calling thread drives the pair itself through persistent
 * device buffers (latency mode). */
int sv_elas_process(sv_handle *h, const uint8_t *I1, const uint8_t *I2, float *D1, float *D2, const int32_t *dims);

/* Test hooks on a live handle (waits for submitted work first).  Keys: "ccl_cap" (runs a band of the speckle stage may hold before a
 * map takes the per-pixel path), "rt_cap" (triangles a raster tile list may hold), "host_force_staging" (host-memory jobs take the
 * pageable route whatever the caller's memory is), "ns_bound" (vertices the next resident launches request LDS for: smaller sets than
 * the chunk has are handed to the host stage), "pool_sleep" (latency handles: pool threads sleep instead of polling), "lat_trace"
 * (wall-clock split of the latency path, printed by sv_destroy), "dma_selftest_fail" (the DMA lanes' self-test reports a failure: the
 * runtime's copies take over); single pairs: "latency_pin" (0: the polling pool threads stay where the pool runs) [SV_LATENCY_PIN],
 * "lat_runtime_copies" (lattice / blob copies through hipMemcpyAsync instead of the copy kernel) [SV_LAT_RUNTIME_COPIES],
 * "lat_filter_alone" (the lattice filters on the calling thread alone) [SV_LAT_FILTER_ALONE]; SV_LAT_WAKE_LEAD_US: how long before a
 * frame that is due the sleeping helpers poll again (default: period / 16 within 0.3 - 2 ms).  Returns SV_OK or SV_ERR_ARG for an unknown key. */
int sv_debug_set(sv_handle *h, const char *key, int value);

/* Test hook: hands the second half of the engine (L/R check, speckle removal, gap interpolation, adaptive mean, median) maps of the
 * caller's choice.  stage "wta": in place of dense_match's maps, in front of the L/R check; "lr": in place of the L/R check's maps, in
 * front of speckle removal.  left / right: float [Hm][Wm] each, the layout sv_debug_get reports for wta1/2 and lr1/2; they are copied
 * into the handle and overwrite the device maps of every later pair that the debug snapshots describe and that has three or more
 * support points, before that stage's snapshot is taken (sv_debug_get returns what was injected).  left == right == NULL clears them.
 * Only on a keep_debug handle (waits for submitted work first); a handle without keep_debug executes nothing of this.
 * Value contract - only what the engine itself can produce at that stage, anything else is refused here on the host, so that a painted
 * map never drives a kernel outside the range it was written for:
 *   "lr"  : -10.0f, or an integer-valued float in 0 .. disp_max (the labelling relies on every invalid pixel being exactly -10);
 *   "wta" : an integer in 0 .. disp_max, or one of dense_match's two invalid values: -10 (no triangle / low texture), -1 (no match).
 * Returns SV_OK, or SV_ERR_ARG with a text for sv_last_error (no keep_debug, unknown stage, one map missing, a value outside the contract). */
int sv_debug_inject(sv_handle *h, const char *stage, const float *left, const float *right);
/* The third stage of that hook, "lattice", with a signature of its own (the lattice is 16-bit): one int16 [Hc][Wc] support lattice,
 * row-major like the dcan_raw snapshot, wc x hc = the handle's lattice size (sv_debug_get "dcan_dims").  Phase 1 of every later chunk
 * copies it, in stream order, over the support matching's lattice of the chunk's last pair (the one the snapshots describe) before
 * the lattice filters run and before the lattice is downloaded: the GPU filters, the host filters and dcan_raw all see it.  It stays
 * staged beside a "wta" / "lr" injection; lattice == NULL, or sv_debug_inject(h, stage, NULL, NULL), clears it.
 * Value contract - what the support matching can leave behind: -1 or an integer in 0 .. disp_max, lattice row 0 and column 0 all zero.
 * Returns SV_OK, or SV_ERR_ARG with a text (no keep_debug, another lattice size, a value outside the contract). */
int sv_debug_inject_lattice(sv_handle *h, const int16_t *lattice, int wc, int hc);

/* Per-stage intermediates of the last pair processed (cfg.keep_debug != 0).  Names and layouts follow
 * oracle/elas_oracle.h: desc1 desc2 dcan_raw support tri1 tri2 planes1 planes2 grid1 grid2 wta1 wta2 lr1 lr2
 * speckle1 gap1 amean1 final1 ...  Returns the byte count, -1 unknown name, -2 cap too small. */
long sv_debug_size(sv_handle *h, const char *name);
long sv_debug_get(sv_handle *h, const char *name, void *out, long cap);

/* Work counters of the two matching kernels (separate instantiations of the kernels; off by default).  mode 1: enable and
 * reset, 0: disable, -1: leave as is; out (may be NULL) receives uint64[8] = {dense candidates evaluated (16-byte SADs),
 * dense pixels matched, support energies evaluated (64-byte SADs), pixels whose plane band took the straight-line path /
 * the scalar-bounded path / the per-lane path of dense_match, trips of its grid-candidate loop per wavefront / per lane (two
 * candidates per trip: lane trips / (64 x wavefront trips) = lane utilisation of that loop)} since the last reset.  Waits for submitted work. */
int sv_debug_counters(sv_handle *h, int mode, uint64_t *out);

/* Per-kernel device timings (HIP events on the worker streams) accumulated since the last reset.
 * names/ms/calls are parallel arrays written up to cap entries; returns the number of kernels known. */
int sv_kernel_times(sv_handle *h, const char **names, double *total_ms, int64_t *calls, int cap);
void sv_kernel_times_reset(sv_handle *h);
void sv_kernel_timing_enable(sv_handle *h, int on);
/* Restricts the timing to the named kernels ("dense_match,support_match", names as sv_kernel_times reports them; NULL or ""
 * = all): every timed launch costs two event records on its stream (all kernels timed: 1-2 % of the throughput). */
int sv_kernel_timing_select(sv_handle *h, const char *names);

/* Host-side stages exposed for tests (they run on the CPU in the product as well, between the two GPU phases):
 * the in-place support-point filters + corner points (elas.cpp:152-264, 413-433) and the Delaunay
 * triangulation (elas.cpp:442-501 -> Triangle "zQB"). */
int sv_host_support_filter(const sv_params *p, int16_t *dcan, int width, int height, int32_t *support, int cap);
/* The same filters with the lattice shared between `threads` threads, as single-pair calls do with the pool threads that sit next to the
 * calling thread (csrc/host_stage.cpp: the order-dependent filter splits into a parallel classification and a short serial pass). */
int sv_host_support_filter_threads(const sv_params *p, int16_t *dcan, int width, int height, int32_t *support, int cap, int threads);
/* Test hook: the same filters by the six kernels of the GPU lattice filter (csrc/kernels.hip: k_filter_*), without a handle, on the current
 * device.  lattices: int16 [n][Hc][Wc], row-major like dcan above and the dcan_raw snapshot, n lattices of one size filtered by ONE
 * launch of each kernel in a workspace the call allocates; prime (may be NULL): n more lattices that go through the same workspace and
 * output buffers first and whose results are dropped.  Out: support int32 [n][cap][3] (the first counts[i] triples of list i),
 * counts int32 [n], stats (may be NULL) int32 [n][3] = {uncertain points after the classification, refinement rounds run, points left
 * to the sequential rest (0 when the rounds settle everything)} of the resolve step.
 * Returns SV_OK; SV_ERR_ARG with a text for sv_last_error(NULL), and nothing runs, for what sv_create keeps on the host
 * (incon_window_size > 5, incon_min_support > 60, incon_threshold >= 4096, a lattice beyond the resolve step's block table), for
 * cap < (Wc-1)*(Hc-1)+6, for a lattice value outside -1 .. disp_max, and for a lattice whose row 0 or column 0 is not all zero (the
 * support matching never writes there); SV_ERR_HIP for a failed HIP call. */
int sv_gpu_support_filter(const sv_params *p, const int16_t *lattices, const int16_t *prime, int n, int width, int height, int32_t *support, int cap, int32_t *counts,
                          int32_t *stats);
int sv_host_delaunay(const int32_t *xy, int n, int32_t *tri_out, int cap);
/* Test hook: exhaustive comparison, on the current device, of the adaptive-mean kernel's division shortcut (v_rcp_f32 + one FMA
 * correction; kernels.hip: amean_div) with the IEEE division: every float mantissa, both signs, 31 exponents, the sixteen divisors
 * a weight sum can be.  Returns the number of differing quotients (0 = the shortcut is exact), < 0 on a HIP error;
 * *control = the same count for a * rcp(d) without the correction (non-zero: the comparison can fail). */
long long sv_debug_check_amean_div(unsigned int *first_a_bits, unsigned int *first_d_bits, long long *control);
/* Same triangulation with the two halves of the top-level cut built by two threads, as the engine does in latency mode
 * (chunk = 1); helper_delay_us > 0 delays the helper thread so that the caller ends up doing both halves itself. */
int sv_host_delaunay_split(const int32_t *xy, int n, int32_t *tri_out, int cap, int helper_delay_us);
/* Same with `depth` levels of the recursion shared (2: four quarters on four threads, what a latency handle with >= 7 pool
 * threads does). */
int sv_host_delaunay_par(const int32_t *xy, int n, int32_t *tri_out, int cap, int depth, int helper_delay_us);
/* Test hook: the divide-and-conquer phase of that triangulation on the GPU (csrc/delaunay_gpu.hip; sort, duplicate scan and k-d
 * ordering on the host), `reps` copies of the set in one launch, kernel time in *kernel_ms (may be NULL).  n <= 4000: one workgroup per set, mesh in LDS;
 * larger sets (<= 256 000): subtrees in LDS, upper merges in a global-memory mesh (SV_DG_SUBMAX lowers the 4000 for tests). */
int sv_gpu_delaunay(const int32_t *xy, int n, int32_t *tri_out, int cap, int reps, double *kernel_ms);

/* Test hook (no GPU needed): the size of the host pool a handle gets by default in this process (cgroup CPU quota or affinity mask,
 * shared between LOCAL_WORLD_SIZE ranks; a mask already as narrow as one rank's share is not divided again).  ignore_quota != 0: as
 * on a host without a CPU quota. */
int sv_default_host_threads(int ignore_quota);

/* Test hooks: the preparation of a vertex set for the triangulation - (x, y) sort, duplicate scan, k-d order (reference:
 * triangle.cpp:5183-5360, 5889-5903) - on the host and on the GPU (csrc/delaunay_gpu.hip: dg_prepare; vertices on the support lattice
 * of a width x height image with lattice step `step` and disparities <= disp_max, n <= 4096).  Both write the ids of the m surviving
 * vertices in the order the divide-and-conquer recursion consumes them and return m.  Coincident vertices: the host keeps the one the
 * reference's quicksort puts first; the GPU form keeps the lowest id when they carry the same disparity (disp[i], may be NULL = unknown)
 * - they are then the same support point twice and interchangeable - and returns -1 (a set it leaves to the host) otherwise. */
int sv_host_kd_order(const int32_t *xy, int n, int32_t *ids_out);
int sv_gpu_kd_order(const int32_t *xy, const int32_t *disp, int n, int width, int height, int step, int disp_max, int32_t *ids_out);

/* ---- (C) calibrated stereo rig: camera frames -> the engine's input ------------------------------------------- */

/* A rig is one calibrated stereo camera: the calibration, Q, and the rectification maps at the matching size.  Any number of
 * rigs can live in one process, independent of each other and of the engine handles.  Its front end turns B pairs of camera
 * frames into the gray, matching-size (and optionally rectified) u8 images sv_process_batch_device takes, with the arithmetic
 * of the legacy entry (stereo_vision.cpp:338-341, 590-591, restated): cv::resize(INTER_LINEAR, exact 2x = INTER_AREA) per
 * channel when the frame's size differs, cvtColor(...2GRAY) with 15-bit weights, cv::remap(INTER_LINEAR, border 0). */
typedef enum sv_pixel_format { SV_PIX_BGRA8 = 0, SV_PIX_BGR8 = 1, SV_PIX_RGB8 = 2, SV_PIX_GRAY8 = 3 } sv_pixel_format;

typedef struct sv_rig sv_rig;

typedef struct sv_rig_config {
    int32_t width, height; /* matching size: the engine's limits, 32..8192 x 32..4096 */
    int32_t device;        /* HIP device of the front end's maps */
    int32_t rectify;       /* 0: off (the reference's default: stereo_vision.cpp:341 is commented out), 1: remap */
    float scale;           /* > 0: K1/K2's first two rows are divided by it (stereo_vision.cpp:364-376) */
    int32_t reserved[3];   /* must be 0 */
} sv_rig_config;

/* Host only (touches no device): parses the OpenCV YAML (K1 K2 D1 D2 R T required, XR XT optional), stereoRectify at the
 * matching size (alpha 0, CALIB_ZERO_DISPARITY) and, with rectify = 1, initUndistortRectifyMap for both cameras.  A bad
 * argument or file returns SV_ERR_ARG; sv_rig_last_error(NULL) gives the text. */
int sv_rig_create(const char *calibration_yaml, const sv_rig_config *cfg, sv_rig **out);
int sv_rig_destroy(sv_rig *r);
/* Text of the last failure on r; r == NULL: of the last failed sv_rig_create on this thread. */
const char *sv_rig_last_error(const sv_rig *r);
/* Q (row major 4x4) and the robot-frame transform XR (3x3) / XT (3) if the file has them; any pointer may be NULL.  Returns a
 * bit mask of what the file had (1 = XR, 2 = XT), or SV_ERR_ARG. */
int sv_rig_matrices(const sv_rig *r, double *Q16, double *XR9, double *XT3);
/* The float maps [4][height][width] = lmapx lmapy rmapx rmapy; SV_ERR_STATE if rectification is off. */
int sv_rig_maps(const sv_rig *r, float *maps);
/* Front end of B pairs, enqueued on `stream` (a hipStream_t, NULL = the default stream) and not waited for.
 *   left / right        : device, B frames back to back, each src_height rows of src_pitch bytes, pixel_format pixels
 *   src_width/height    : the frames' size (<= 2^26 pixels); another size than the matching one is resized to it
 *   gray_left/right     : device u8 [B][height][width] (the matching size)
 *   left_bgra           : device u8 [B][height][width][4], 4-byte aligned, or NULL: the left image at the matching size before
 *                         the remap, as BGRA (A = 255 for 3-channel and gray sources) - the colours getColor() returns
 * The first call with rectification uploads the maps to cfg.device.  Calls on one rig are serialised; work from several rigs
 * may interleave freely.  Returns SV_OK, SV_ERR_ARG (nothing enqueued), SV_ERR_NO_DEVICE or SV_ERR_HIP. */
int sv_rig_frontend_device(sv_rig *r, const uint8_t *left, const uint8_t *right, int batch, int src_width, int src_height, int src_pitch, int pixel_format,
                           uint8_t *gray_left, uint8_t *gray_right, uint8_t *left_bgra, void *stream);

/* ---- (D) bird's-eye views: point clouds or disparity maps -> 2-D ground grids ---------------------------------- */

/* The grid of the reference's points_2_top_view (stereo_vision/sv.py:87-134), restated in our stereo_vision/sv.py.  The axes are
 * lidar axes: x forward becomes the rows, y left the columns.  For each point (X, Y, Z) of a frame, in double:
 *   in range  x0 < X < x1 && y0 < Y < y1 && z0 < Z < z1 (strict: NaN and +-inf never pass)
 *   cell      row = trunc(x1 s) - trunc(X s), col = trunc(y1 s) - trunc(Y s) (every in-range point lands in the grid)
 *   value     (uint8) trunc(((max_dist - dist) / max_dist) * 255) with dist = sqrt(X*X + Y*Y), max_dist = sqrt(x1*x1 + y1*y1)
 *             (no FMA, correctly rounded sqrt); 0 where dist > max_dist (the reference's cast of a negative is undefined)
 * SV_TOPVIEW_REFERENCE: uint8 [B][rows][cols], each cell the value of its in-range point with the largest flat index (numpy's
 * last-writer order of img[y_img, x_img] = dist_lim), 0 where empty.  SV_TOPVIEW_COUNT: int32 [B][rows][cols], the number of
 * in-range points per cell.  Both are bitwise reproducible. */
enum { SV_TOPVIEW_REFERENCE = 0, SV_TOPVIEW_COUNT = 1 };
enum { SV_TOPVIEW_DMAP = 0, SV_TOPVIEW_D1 = 1 };

typedef struct sv_top_view_spec {
    double x_range[2], y_range[2], z_range[2]; /* x/y: integer-valued, lo < hi, |bound| <= 2^31; z: lo < hi (may be infinite) */
    int32_t scale;                              /* >= 1 */
    int32_t mode;                               /* SV_TOPVIEW_REFERENCE = 0 (u8), SV_TOPVIEW_COUNT = 1 (int32) */
    int32_t disparity;                          /* SV_TOPVIEW_DMAP = 0, SV_TOPVIEW_D1 = 1 (disparity entry only) */
    int32_t reserved[5];                        /* must be 0 */
} sv_top_view_spec;

/* Host only: rows = (x1 - x0) * scale + 1, cols = (y1 - y0) * scale + 1.  SV_ERR_ARG for a bad spec: a NULL spec or output, a
 * non-integer, non-finite or too large x / y bound, lo >= hi (NaN included), scale < 1, mode or disparity not 0 / 1, a non-zero
 * reserved word, a grid over 32768 in either dimension, or max_dist == 0 in reference mode (x1 = y1 = 0). */
int sv_top_view_dims(const sv_top_view_spec *spec, int *rows, int *cols);
/* Host only: bytes of the uint64 [batch][rows][cols] workspace reference mode needs; 0 in count mode; SIZE_MAX for a bad spec or
 * batch < 0. */
size_t sv_top_view_workspace_bytes(const sv_top_view_spec *spec, int batch);
/* Grids of a batch of f64 clouds, enqueued on `stream` (a hipStream_t, NULL = the default stream) and not waited for.
 *   points     : double [batch][n_points][3] device; n_points < 2^31
 *   out        : device, uint8 (reference) or int32 (count) [batch][rows][cols]; every cell is written
 *   workspace  : device, >= sv_top_view_workspace_bytes(spec, batch) bytes, 8-byte aligned (may be NULL in count mode)
 * batch <= 65535.  Returns SV_OK (batch 0: nothing enqueued), SV_ERR_ARG (bad spec, NULL buffer, workspace too small, n_points out
 * of range; nothing enqueued) or SV_ERR_HIP. */
int sv_top_view_points_device(const double *points, int batch, int64_t n_points, const sv_top_view_spec *spec, void *out, void *workspace,
                              size_t workspace_bytes, void *stream);
/* The same from disparity maps, fused: each pixel's point is computed in registers with sv_reproject_batch_device's arithmetic and
 * summation order, and no cloud is written.  spec->disparity: SV_TOPVIEW_DMAP reprojects the driver's dmap = saturate(
 * round_half_even(4 d)) of every pixel, so the grid equals that of sv_reproject_batch_device's cloud (its points are at a quarter of
 * metric depth: the driver's convention); SV_TOPVIEW_D1 reprojects the float d itself (metres) and skips pixels with d <= 0 (the
 * engine's invalid pixels are -10).  The flat index of pixel (x, y) is y * width + x.
 *   disp       : float [batch][height][width] device; width * height < 2^31, height <= 65535
 *   Q16, XR9, XT3: HOST, as for sv_reproject_batch_device (XR9 and XT3 both NULL = no transform)
 * Other arguments and results as sv_top_view_points_device. */
int sv_top_view_disparity_device(const float *disp, int batch, int width, int height, const double *Q16, const double *XR9, const double *XT3,
                                 const sv_top_view_spec *spec, void *out, void *workspace, size_t workspace_bytes, void *stream);
/* Test hook for the calls above, process-wide: combine != 0 (the default) merges the lanes of a wavefront that hit the same cell
 * into one atomic; atomics_device != NULL: every grid atomic issued is also counted into that device uint64.  Returns SV_OK. */
int sv_debug_top_view(int combine, unsigned long long *atomics_device);

/* ---- (E) object positions: disparity maps or point clouds + detector boxes -> one 3-D point per box --------------- */

/* What publishPointCloud computes for every tracked object (stereo_vision.cpp:261-278: the mean of the cloud inside the detector's
 * box), for B pairs with up to max_boxes boxes each, and beside the reference's plain mean two selections that survive invalid pixels
 * and background.  The boxes are the caller's (no detector is part of this library).
 *
 * Box: (x, y, w, h) int32, pixels of the width x height map.  Its pixels are the columns i in [clamp(x), clamp(x + w)) and the rows j
 * in [clamp(y), clamp(y + h)) with clamp(a) = min(max(a, 0), size - 1), as in the reference (:263-264) and in sv_legacy_box_means: the
 * map's last column and last row are never part of a box.  x + w and y + h are formed in 64 bits.  A box without a pixel (w <= 0,
 * h <= 0, wholly outside) is legal: n_pixels = 0.
 *
 * Pixel: q = its quantised disparity in quarter pixels, P = its point, both with sv_reproject_batch_device's arithmetic (no FMA):
 *   SV_BOX_DMAP  q = saturate_u8(round_half_even(4 d)) (0..255; NaN gives 0), P = reproject(i, j, (double)q) (+ XR / XT): the driver's
 *                cloud, at a quarter of metric depth.  Valid iff q > 0.
 *   SV_BOX_D1    q = min(round_half_even(4 d), 4095) (4 d in float), P = reproject(i, j, (double)d) (+ XR / XT), in metres.  Valid
 *                iff d > 0 (NaN is invalid; the engine's invalid pixels are -10).
 *
 * Selection:
 *   SV_BOX_ALL    every pixel of the box - the reference's mean; inf / NaN propagate as IEEE says (a pixel with q = 0 has pos.w = 0).
 *                 With SV_BOX_DMAP this is sv_legacy_box_means for a batch.
 *   SV_BOX_VALID  the valid pixels.
 *   SV_BOX_NEAR   the valid pixels with |q - q_med| <= band; q_med = the lower median of q over the box's valid pixels (the smallest q
 *                 whose cumulative count reaches (n_valid + 1) / 2), band >= 0 in quarter pixels.
 *
 * Results per box:
 *   pos   double [3] = (sum of P over the selected pixels) / (double)n_selected; nothing selected: 0.0 / 0.0 = NaN, as the reference's
 *         division gives
 *   stat  int32 [4] = (n_pixels, n_valid, q_med or -1 when n_valid == 0, n_selected), the same for every selection.  The points
 *         entry knows no disparity: (n_pixels, -1, -1, n_pixels).
 *
 * Summation order (per coordinate; the doubles are bitwise reproducible and independent of the batch, of the other boxes, of their
 * order and of the launch): for each column of the box, left to right, the selected points are added in ascending row order onto
 * +0.0 (unselected pixels are skipped, not added as zeros); the column sums - of every column, 0.0 where nothing was selected - are then
 * added left to right onto +0.0.  stereo_vision.sv.box_positions restates it in numpy.  The reference (and sv_legacy_box_means) keeps
 * ONE running accumulator over columns outer / rows inner, so SV_BOX_ALL agrees with it to rounding: identical for a box one column
 * wide, otherwise both are recursive sums of the same n terms and per coordinate |ours - theirs| <= 2 g sum|P_i| with
 * g = (n - 1) u / (1 - (n - 1) u), u = 2^-53; a sum that is not finite has the same class (+inf, -inf, NaN) in both. */
enum { SV_BOX_ALL = 0, SV_BOX_VALID = 1, SV_BOX_NEAR = 2 };
enum { SV_BOX_DMAP = 0, SV_BOX_D1 = 1 };

typedef struct sv_box_spec {
    int32_t select;      /* SV_BOX_ALL / SV_BOX_VALID / SV_BOX_NEAR */
    int32_t disparity;   /* SV_BOX_DMAP / SV_BOX_D1 (read by the disparity entry; must be one of them for the points entry too) */
    int32_t band;        /* >= 0, quarter pixels (SV_BOX_NEAR) */
    int32_t reserved[5]; /* must be 0 */
} sv_box_spec;

/* From disparity maps, fused: each pixel's point is computed in registers and no cloud is written.  Enqueued on `stream` (a
 * hipStream_t, NULL = the default stream) as ONE kernel and not waited for; nothing is allocated; safe under stream capture.
 *   disp         : float [batch][height][width] device; width * height < 2^31
 *   Q16, XR9, XT3: HOST, as for sv_reproject_batch_device (XR9 and XT3 both NULL = no transform)
 *   boxes        : int32 [batch][max_boxes][4] device
 *   n_boxes      : int32 [batch] device, or NULL = max_boxes each.  A value outside [0, max_boxes] is clamped by the kernel (it is
 *                  device data the host does not read).  Rows of boxes at and beyond n_boxes[b] are left untouched in pos / stat.
 *   pos          : double [batch][max_boxes][3] device
 *   stat         : int32 [batch][max_boxes][4] device, or NULL
 * Returns SV_OK (nothing enqueued for batch == 0 or max_boxes == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs
 * untouched, the text in sv_last_error(NULL) - for: a NULL spec, disp, Q16, boxes or pos; select or disparity out of range;
 * band < 0; a non-zero reserved word; batch < 0 or > 65535; max_boxes < 0 or > 65535; width < 1 or height < 1;
 * width * height >= 2^31. */
int sv_box_positions_disparity_device(const float *disp, int batch, int width, int height, const double *Q16, const double *XR9, const double *XT3,
                                      const int32_t *boxes, const int32_t *n_boxes, int max_boxes, const sv_box_spec *spec, double *pos, int32_t *stat,
                                      void *stream);
/* The same over f64 clouds: points double [batch][height][width][3] device (e.g. sv_reproject_batch_device's points_out), SV_BOX_ALL
 * only - a cloud has no disparity to select by; any other selection is SV_ERR_ARG, as is a NULL points.  Other arguments, results and
 * errors as above.  On sv_reproject_batch_device's cloud it returns what the disparity entry returns for SV_BOX_ALL, SV_BOX_DMAP, bit
 * for bit. */
int sv_box_positions_points_device(const double *points, int batch, int width, int height, const int32_t *boxes, const int32_t *n_boxes, int max_boxes,
                                   const sv_box_spec *spec, double *pos, int32_t *stat, void *stream);

/* ---- (F) compact coloured point clouds: disparity maps (+ colour images) -> lists of points per pair ----------------- */

/* The points a viewer, a PLY file or a voxel grid takes: for B pairs, the 3-D points of the pixels that carry a disparity and lie
 * inside a crop box, optionally thinned out to every step-th column and row, each with its colour and its pixel index.
 *
 * Frame b visits the pixels (x, y) with x % step == 0 && y % step == 0 in ascending flat index y * width + x.  All arithmetic is
 * sv_reproject_batch_device's (double, no FMA):
 *   SV_CLOUD_DMAP  q = saturate_u8(round_half_even(4 d)) (NaN gives 0); candidate iff q > 0; P = reproject(x, y, (double)q): the
 *                  driver's cloud, at a quarter of metric depth (as in (D) and (E)).
 *   SV_CLOUD_D1    candidate iff d > 0 (NaN is none; the engine's invalid pixels are -10); P = reproject(x, y, (double)d), metres.
 *   XR9 / XT3      P = XR P + XT, as everywhere else.
 *   crop           after the transform: a candidate is kept iff lo[k] < P[k] < hi[k] for k = 0, 1, 2, strictly.  lo = -inf /
 *                  hi = +inf leave an axis open.  +-inf and NaN coordinates never pass, even with every axis open - so "d > 0" alone
 *                  is not the predicate: a Q that makes pos.w = 0 for some positive disparity yields no point there.
 * A kept point is written as
 *   xyz    SV_CLOUD_F32: (float)P, IEEE round to nearest even (a coordinate beyond the float range becomes +-inf although it passed
 *          the crop in double); SV_CLOUD_F64: P itself
 *   color  the four bytes of pixel (x, y) of `colors` (e.g. sv_rig_frontend_device's BGRA output); optional
 *   index  int32 y * width + x; optional
 * counts[b] is the number of kept points of frame b, NOT capped by the capacity.  The frame's first min(counts[b], capacity) kept
 * points, in pixel order, land in rows 0.. of the frame's slot; the rows beyond are left untouched.  The result of a frame is
 * bitwise reproducible and independent of the batch it sits in, of the launch and of the other frames.
 * stereo_vision.sv.compact_cloud restates all of it in numpy. */
enum { SV_CLOUD_DMAP = 0, SV_CLOUD_D1 = 1 };
enum { SV_CLOUD_F32 = 0, SV_CLOUD_F64 = 1 };

typedef struct sv_cloud_spec {
    double lo[3], hi[3];  /* lo < hi per axis (NaN refused); infinite = open */
    int32_t disparity;    /* SV_CLOUD_DMAP / SV_CLOUD_D1 */
    int32_t step;         /* >= 1: every step-th column and row */
    int32_t dtype;        /* SV_CLOUD_F32 / SV_CLOUD_F64 */
    int32_t reserved[5];  /* must be 0 */
} sv_cloud_spec;

/* Visited pixels per tile, the unit the kernels count and write by (a test hook: shapes around it are the edges of the tiling). */
int sv_cloud_tile(void);
/* Bytes of device workspace a call needs (4 per tile and pair; 0 for batch == 0).  Host only; SIZE_MAX for a bad spec, batch, width or
 * height (the checks of the call below). */
size_t sv_cloud_workspace_bytes(const sv_cloud_spec *spec, int batch, int width, int height);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as at most three kernels - count per tile, scan per frame, write -
 * and not waited for; nothing is allocated, no host synchronisation is made.
 *   disp         : float [batch][height][width] device; width * height < 2^31
 *   colors       : uint8 [batch][height][width][4] device, 4-byte aligned, or NULL
 *   Q16, XR9, XT3: HOST, as for sv_reproject_batch_device (XR9 and XT3 both NULL = no transform)
 *   capacity     : rows per pair of the three outputs, >= 0; 0: only the counts are produced (two kernels; xyz may be NULL)
 *   xyz          : float or double [batch][capacity][3] device
 *   color_out    : uint8 [batch][capacity][4] device, 4-byte aligned, or NULL; needs colors
 *   index_out    : int32 [batch][capacity] device, or NULL
 *   counts       : int32 [batch] device
 *   workspace    : device, 4-byte aligned, workspace_bytes >= sv_cloud_workspace_bytes(spec, batch, width, height); its contents
 *                  before and after the call mean nothing
 * Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in
 * sv_last_error(NULL) - for: a NULL spec, disp, Q16 or counts; a NULL xyz with capacity > 0; color_out without colors; colors or
 * color_out not 4-byte aligned; disparity or dtype out of range; step < 1; lo >= hi or a NaN bound; a non-zero reserved word;
 * a workspace that is NULL, misaligned or too small; capacity < 0; batch < 0 or > 65535; width < 1 or height < 1;
 * width * height >= 2^31.  These checks run before any HIP call. */
int sv_cloud_disparity_device(const float *disp, const uint8_t *colors, int batch, int width, int height, const double *Q16, const double *XR9,
                              const double *XT3, const sv_cloud_spec *spec, int capacity, void *xyz, uint8_t *color_out, int32_t *index_out, int32_t *counts,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---- (G) ground plane, obstacle labels and free space: disparity maps -> a line, labels and a row per column ---------- */

/* Where the ground is, what stands on it and how far one can go in each image column, for B pairs: Labayrade's v-disparity line fit
 * followed by a per-column scan.  Integer work throughout; the results are bitwise reproducible and independent of the batch a pair sits
 * in.  stereo_vision.sv (v_disparity, ground_line, ground_labels, free_space) restates all of it in numpy.
 *
 *   bins       a pixel is valid iff d > 0 (NaN is not; the engine's invalid pixels are -10); its bin is
 *              q = min(rintf(4.0f * d), n_bins - 1): quarter pixels, round half to even - the only floating-point operations.
 *   vdisp      vdisp[b][v][q] = the number of valid pixels of row v in bin q.
 *   ground     the line through (row vh, bin 0) - the horizon - and (row height - 1, bin qb): with den = height - 1 - vh
 *                ql(v) = (2 qb (v - vh) + den) / (2 den), integer division (v > vh: nothing is negative)
 *                S(vh, qb) = sum over v = max(vh + 1, 0) .. height - 1 and k = -tol .. tol with 0 <= ql(v) + k < n_bins of vdisp[b][v][ql(v) + k]
 *              over the candidates vh = vh_lo, vh_lo + vh_step, ... <= vh_hi and qb = qb_step, 2 qb_step, ... < n_bins.  The largest S
 *              wins; ties go to the smallest vh, then the smallest qb.  ground[b] = {vh, qb, S, n_valid} (n_valid = the valid pixels
 *              of the map), or {-1, -1, S, n_valid} - "no ground" - when S < min_support (an all-invalid map has S = 0).
 *   labels     with g(v) = ql(v) for v > vh, 0 for v <= vh, and e = q - g(v):
 *                0 invalid, 1 ground (|e| <= g_tol), 2 obstacle (e > g_tol), 3 below the ground (e < -g_tol);
 *              with "no ground" every valid pixel is 3.
 *   free space per column u, walking from row height - 1 upwards: the first row v such that the min_run rows v, v - 1, ...,
 *              v - min_run + 1 exist and are all obstacle; free_row[b][u] = v, free_disp[b][u] = disp[b][v][u]; -1 and 0.0f for a
 *              column without one. */
typedef struct sv_ground_spec {
    int32_t n_bins;       /* 8..4096; 4 * (disp_max + 1) holds every disparity of the engine */
    int32_t vh_lo, vh_hi; /* -32768 <= vh_lo <= vh_hi <= height - 2 */
    int32_t vh_step;      /* >= 1 */
    int32_t qb_step;      /* 1..n_bins - 1: at least one candidate */
    int32_t tol;          /* 0..16: half width of the band that is summed, in bins */
    int32_t g_tol;        /* 0..4096: half width of the band that is labelled ground, in bins */
    int32_t min_run;      /* >= 1: obstacle rows in a column that stop the free space */
    int32_t min_support;  /* >= 0: the least S that is a ground */
    int32_t reserved[7];  /* must be 0 */
} sv_ground_spec;

/* Bytes of device workspace a call needs (8 per candidate vh and 4 (n_bins + 1) per row, per pair; 0 for batch == 0).  Host only;
 * SIZE_MAX for a bad spec, batch, width or height (the checks of the call below). */
size_t sv_ground_workspace_bytes(const sv_ground_spec *spec, int batch, int width, int height);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as four kernels - histogram and prefix sums, search, pick, labels
 * and free space (left out when none of its three outputs is asked for) - and not waited for; nothing is allocated, no host
 * synchronisation is made.
 *   disp         : float [batch][height][width] device
 *   vdisp        : uint32 [batch][height][n_bins] device, or NULL
 *   ground       : int32 [batch][4] device
 *   labels       : uint8 [batch][height][width] device, or NULL
 *   free_row     : int32 [batch][width] device, or NULL
 *   free_disp    : float [batch][width] device, or NULL
 *   workspace    : device, 8-byte aligned, workspace_bytes >= sv_ground_workspace_bytes(spec, batch, width, height); its contents
 *                  before and after the call mean nothing
 * An output left out does not change the others.
 * Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in
 * sv_last_error(NULL) - for: a NULL spec, disp or ground; disp, vdisp, ground, free_row or free_disp not 4-byte aligned; a spec word
 * outside the range given beside it; a non-zero reserved word; a workspace that is NULL, misaligned or too small; batch < 0 or
 * > 65535; width < 1 or height < 1; height > 32768; width * height >= 2^31.  These checks run before any HIP call.
 * The environment variable SV_GROUND_HIST=plain selects the histogram kernel without wavefront aggregation (a measurement aid: the
 * results are the same). */
int sv_ground_disparity_device(const float *disp, int batch, int width, int height, const sv_ground_spec *spec, uint32_t *vdisp, int32_t *ground,
                               uint8_t *labels, int32_t *free_row, float *free_disp, void *workspace, size_t workspace_bytes, void *stream);

/* ---- (H) stixels and detector-free object boxes: disparity maps + obstacle labels -> segments per column, boxes per pair ---- */

/* What stands on the ground as things: per visited image column the vertical segments ("stixels") of obstacle pixels that stay near
 * the disparity of their own base, and objects grouped from the nearest segment of neighbouring columns, as boxes that
 * sv_box_positions_* takes.  Integers only after the bin; the results are bitwise reproducible and independent of the batch, of the
 * launch and of the other pairs.  stereo_vision.sv (stixels, stixel_objects, stixel_world) restates all of it in numpy.
 *
 *   foreground a pixel with labels == 2 (the obstacle label of (G)), d > 0 and q >= q_min, q = min(rintf(4.0f * d), n_bins - 1) - (G)'s
 *              bin, the only floating-point operations.  The labels are the caller's data: a NaN or a -10 under a label 2 is not
 *              foreground.  q_min drops what is too far to matter.
 *   stixels    column u is visited iff u % col_step == 0; the visited columns are numbered i = u / col_step < Wv = ceil(width / col_step).
 *              Walk the column from row height - 1 upwards.  At a foreground row v a run starts with base qb = q[v][u].  A row above
 *              matches iff it is foreground and |q - qb| <= sim - against the base, not the neighbouring row, so a run cannot drift
 *              along a slanted surface.  The run extends upwards over matching rows and bridges rows that do not match; it ends at the
 *              image top or as soon as max_gap + 1 consecutive rows fail to match.  t = its last matching row (t = v if none matched),
 *              n = the number of matching rows, the base included.  n >= min_rows makes the run a stixel
 *              (v_bottom, v_top, q_base, n_rows) = (v, t, qb, n).  Either way the walk continues at row t - 1: bridged rows belong to
 *              the run and are not visited again, rows above t that only ended the run are.  The stixels of a column are its layers
 *              0, 1, ... bottom-up.  n_stixels[b][i] = the column's count, not capped; the first max_layers are stored in
 *              stixels[b][layer][i][4], the entries of layers at and beyond the count are -1.
 *   objects    from layer 0 alone - it is what bounds the free space.  An object is a maximal run of consecutive visited columns that
 *              each have a layer-0 stixel and whose q_base differs from the previous visited column's by at most sim_cols; it is kept iff
 *              it spans at least min_cols visited columns.  Kept objects are listed left to right, two rows of four int32 each:
 *                boxes = (x, y, w, h) = (first column, smallest v_top, last column - first column + 1, largest v_bottom - y + 1), in
 *                        pixels: the box layout of (E).  (E) never counts the map's last column and last row, so a box that reaches
 *                        them loses them there.
 *                info  = (n_cols, q_lo, q_hi, q_med): the visited columns, the smallest and the largest q_base and their lower median,
 *                        by (E)'s rank rule - the smallest value whose cumulative count reaches (n_cols + 1) / 2.
 *              counts[b] = the kept objects, not capped; the first min(counts[b], capacity) are written and the rows beyond are left
 *              untouched, as sv_cloud_* does.  counts can be passed as n_boxes to sv_box_positions_disparity_device with
 *              max_boxes = capacity: that kernel clamps it.
 *   identity   with sim >= n_bins, q_min = 0, max_gap = 0, col_step = 1 and min_rows = (G)'s min_run on (G)'s own labels, v_bottom of
 *              layer 0 equals free_row, -1 ("no stixel") included. */
typedef struct sv_stixel_spec {
    int32_t n_bins;      /* 8..4096; the value given to (G) */
    int32_t q_min;       /* 0..4095: the least bin that is foreground */
    int32_t sim;         /* 0..4096: rows of a run are within sim bins of its base */
    int32_t max_gap;     /* 0..255: consecutive rows a run bridges */
    int32_t min_rows;    /* >= 1: matching rows that make a run a stixel */
    int32_t max_layers;  /* 1..64: stixels stored per column */
    int32_t col_step;    /* >= 1: every col_step-th column is visited */
    int32_t sim_cols;    /* 0..4096: neighbouring columns of an object are within sim_cols bins of each other */
    int32_t min_cols;    /* >= 1: visited columns that make an object */
    int32_t reserved[7]; /* must be 0 */
} sv_stixel_spec;

/* Bytes of device workspace a call needs (16 per visited column, per pair: the first layer; 0 for batch == 0).  Host only; SIZE_MAX
 * for a bad spec, batch, width or height (the checks of the call below). */
size_t sv_stixel_workspace_bytes(const sv_stixel_spec *spec, int batch, int width, int height);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as two kernels - the columns' walk, the objects - and not waited for;
 * nothing is allocated, no host synchronisation is made.  With Wv = ceil(width / col_step):
 *   disp         : float [batch][height][width] device
 *   labels       : uint8 [batch][height][width] device, as sv_ground_disparity_device writes them
 *   stixels      : int32 [batch][max_layers][Wv][4] device, or NULL
 *   n_stixels    : int32 [batch][Wv] device, or NULL
 *   boxes        : int32 [batch][capacity][4] device, or NULL
 *   info         : int32 [batch][capacity][4] device, or NULL
 *   counts       : int32 [batch] device
 *   workspace    : device, 16-byte aligned, workspace_bytes >= sv_stixel_workspace_bytes(spec, batch, width, height); its contents
 *                  before and after the call mean nothing
 * An output left out does not change the others.
 * Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in
 * sv_last_error(NULL) - for: a NULL spec, disp, labels or counts; disp, n_stixels or counts not 4-byte aligned; stixels, boxes or info
 * not 16-byte aligned (a record is stored as one 16-byte word); a spec word outside the range given beside it; a non-zero reserved
 * word; capacity < 0; a workspace that is NULL, misaligned or too small; batch < 0 or > 65535; width < 1 or height < 1;
 * height > 32768; width * height >= 2^31.  These checks run before any HIP call.
 * The environment variable SV_STIXEL_STAGE=columns leaves the second kernel out (a measurement aid: boxes, info and counts are then
 * not written). */
int sv_stixel_disparity_device(const float *disp, const uint8_t *labels, int batch, int width, int height, const sv_stixel_spec *spec, int capacity,
                               int32_t *stixels, int32_t *n_stixels, int32_t *boxes, int32_t *info, int32_t *counts, void *workspace,
                               size_t workspace_bytes, void *stream);

/* ---- (I) voxel clouds: disparity maps (+ colour images) -> one row per occupied cell of a 3-D grid, per pair ------------------- */

/* What registration, mapping, an occupancy grid or a planner takes instead of (F)'s list: a voxel-grid filter over it, fused with it.
 * The grid covers the crop box with cubic cells of edge `size`; unlike (F) the crop is finite.  Per axis k it has
 * n_k = max(1, (int64)ceil((hi_k - lo_k) / size)) cells, at most 2^20 (a cell index fits an int32, the three of them 60 bits).
 *
 *   kept pixels  exactly (F)'s: the visited pixels (x % step == 0 && y % step == 0, ascending flat index y * width + x), the candidate
 *                rule of spec->disparity, P = reproject(x, y, .) in double without FMA, the transform included; kept iff lo < P < hi
 *                strictly on all three axes.
 *   cell         of a kept point, per axis, in double and in this order: t = (P - lo) / size; c = min((int64)t, n - 1);
 *                u = min((int64)((t - (double)c) * 65536.0), 65535) - the offset inside the cell in 1/65536 of its edge.  t >= c >= 0,
 *                so nothing is negative; the two min catch a quotient that rounds up onto n.
 *   voxel        the kept points of a frame with equal (c_x, c_y, c_z).  Per voxel: n = its points, first = the smallest flat pixel
 *                index among them, S_k = sum of u_k and, with colours, C_j = sum of channel j.  All are integers: n and first have 32
 *                bits (width * height < 2^31), S_k <= 65535 n < 2^47 and C_j <= 255 n < 2^39 have 64, so no admitted map overflows them
 *                and the sums do not depend on the order in which the points are met.
 *   rows         a frame's voxels in ascending `first` - the order in which a scan of the image meets them, so a prefix of the list is
 *                the voxels of a prefix of the image.  A row is
 *     xyz[3]     m_k = lo_k + ((double)c_k + ((double)S_k + 0.5 * (double)n) / (65536.0 * (double)n)) * size, evaluated in double as
 *                written, no FMA; SV_CLOUD_F32 stores (float)m_k.  It is the centroid with each point's offset truncated to 1/65536 of
 *                the cell and re-centred: |m_k - true mean| <= size * 2^-17, plus double rounding.
 *     cell[3]    int32 c; n int32; first int32 (each optional)
 *     color[4]   uint8 (2 C_j + n) / (2 n) per channel, integer division: the mean rounded half up (optional; needs colors)
 *   counts[b]    the number V of voxels of frame b if V <= capacity, and -1 if V > capacity: raise the capacity; the frame's rows then
 *                mean nothing.  A function of the input alone.  It is deliberately not (F)'s uncapped count: the table that finds the
 *                voxels is sized by the capacity.  Rows at and beyond counts[b] are left untouched.
 * The result of a frame is bitwise reproducible and independent of the batch it sits in, of the launch, of the other frames and of
 * repetition.  stereo_vision.sv.voxel_cloud restates all of it in numpy. */
typedef struct sv_voxel_spec {
    double lo[3], hi[3];  /* finite, lo < hi per axis */
    double size;          /* finite, > 0: the edge of a cell; ceil((hi - lo) / size) <= 2^20 per axis */
    int32_t disparity;    /* SV_CLOUD_DMAP / SV_CLOUD_D1 */
    int32_t step;         /* >= 1: every step-th column and row */
    int32_t dtype;        /* SV_CLOUD_F32 / SV_CLOUD_F64 */
    int32_t reserved[5];  /* must be 0 */
} sv_voxel_spec;

/* Entries of the open-addressing table a pair gets for `capacity` rows: the power of two >= 2 * max(capacity, 512), 72 bytes each;
 * -1 for a capacity outside 1 .. 2^26. */
int64_t sv_voxel_table_slots(int capacity);
/* Bytes of device workspace a call needs: per pair the table, 16 bytes of counters and one bit per visited pixel (padded to 16 bytes),
 * then (F)'s 4 bytes per tile and pair; 0 for batch == 0.  Host only; SIZE_MAX for a bad spec, batch, width, height or capacity (the
 * checks of the call below). */
size_t sv_voxel_workspace_bytes(const sv_voxel_spec *spec, int batch, int width, int height, int capacity);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as six kernels - clear the tables, insert the points, mark each
 * voxel's first pixel, count the marks per tile, (F)'s scan per frame, write the rows - and not waited for; nothing is allocated, no
 * host synchronisation is made.
 *   disp         : float [batch][height][width] device; width * height < 2^31
 *   colors       : uint8 [batch][height][width][4] device, 4-byte aligned, or NULL
 *   Q16, XR9, XT3: HOST, as for sv_reproject_batch_device (XR9 and XT3 both NULL = no transform)
 *   capacity     : rows per pair of the outputs, 1 .. 2^26
 *   xyz          : float or double [batch][capacity][3] device
 *   color_out    : uint8 [batch][capacity][4] device, 4-byte aligned, or NULL; needs colors
 *   cell_out     : int32 [batch][capacity][3] device, or NULL
 *   n_out        : int32 [batch][capacity] device, or NULL
 *   first_out    : int32 [batch][capacity] device, or NULL
 *   counts       : int32 [batch] device
 *   workspace    : device, 16-byte aligned, workspace_bytes >= sv_voxel_workspace_bytes(spec, batch, width, height, capacity); its
 *                  contents before and after the call mean nothing
 * An output left out does not change the others.
 * Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in
 * sv_last_error(NULL) - for: a NULL spec, disp, Q16, counts or xyz; color_out without colors; colors or color_out not 4-byte aligned;
 * disparity or dtype out of range; step < 1; a bound of the crop that is not finite; lo >= hi; a size that is not finite or <= 0; more
 * than 2^20 cells on an axis; a non-zero reserved word; capacity < 1 or > 2^26; a workspace that is NULL, misaligned or too small;
 * batch < 0 or > 65535; width < 1 or height < 1; width * height >= 2^31.  These checks run before any HIP call.
 * The environment variable SV_VOXEL_STAGE = clear, insert, mark or scan leaves out the kernels behind that stage (a measurement aid:
 * the rows, and before "scan" the counts, are then not written). */
int sv_voxel_disparity_device(const float *disp, const uint8_t *colors, int batch, int width, int height, const double *Q16, const double *XR9,
                              const double *XT3, const sv_voxel_spec *spec, int capacity, void *xyz, uint8_t *color_out, int32_t *cell_out, int32_t *n_out,
                              int32_t *first_out, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);
/* Test hook for the call above, process-wide: combine != 0 (the default) merges the lanes of a wavefront that hold neighbouring
 * pixels of one cell into one table update; counters_device != NULL: a device uint64 [2] that receives [0] the table updates issued
 * (without the merge: one per kept point) and [1] the atomic instructions issued for them (per update one compare-and-swap per probed
 * slot, 5 or, with colours, 9 sums, and 1 or 2 for a claimed slot).  The results do not depend on it.  Returns SV_OK. */
int sv_debug_voxel(int combine, unsigned long long *counters_device);

/* ---- (J) occupancy and elevation grids: disparity maps + labels + free space -> evidence, sight lines and a state per cell ---- */

/* What a planner takes: per cell of (D)'s bird's-eye grid the ground and obstacle pixels that fell into it, the height span of what
 * was seen there, the number of sight lines that crossed it and a state - unknown, free or occupied - for B pairs.  "Seen and empty"
 * (a sight line crossed the cell) is told from "never seen".  Integers from the cell index on; the results are bitwise reproducible
 * and independent of the batch, of the launch and of the other pairs.  stereo_vision.sv.occupancy_grid restates all of it in numpy.
 *
 *   grid       (D)'s in SV_TOPVIEW_COUNT mode, with (D)'s checks: rows = (x1 - x0) scale + 1, cols = (y1 - y0) scale + 1; a point (X, Y)
 *              lies in cell (R1 - trunc(X s), C1 - trunc(Y s)), R1 = trunc(x1 s), C1 = trunc(y1 s), products in double.
 *   evidence   a pixel counts iff d > 0 (NaN does not) and its label is 1 (ground) or 2 (obstacle) - (G)'s labels; 0 and 3 never count,
 *              so a pair without ground (every valid pixel 3) yields an all-unknown grid.  Its point is P = reproject(x, y, (double)d)
 *              (+ XR / XT), double, no FMA, as SV_TOPVIEW_D1; it is kept iff x0 < X < x1, y0 < Y < y1, z0 < Z < z1, strictly (inf and NaN
 *              drop out).  Its height is h = min(trunc((Z - z0) * z_scale), 65535): z_scale height steps per metre, an integer, so no
 *              division stands between Z and h.
 *   cells      int32 [4] per cell = (n_ground, n_obstacle, h_lo, h_hi): the kept pixels of either label, and the smallest and the
 *              largest h over both; h_lo = h_hi = -1 for a cell without one.
 *   n_rays     per image column u one sight line from the origin cell (R1 - trunc(Ox s), C1 - trunc(Oy s)), O = XT3 or 0 - the camera
 *              centre in the caller's frame; it is not range-tested and may lie outside the grid - to the cell of
 *                free_row[u] >= 0: the point of pixel (u, free_row[u]) with disparity free_disp[u] - the obstacle's base.  Only the three
 *                                  numbers are used; no pixel is read.
 *                free_row[u] < 0 : the point of the topmost pixel of the column with label 1 and d > 0 - a ground end; a column without
 *                                  such a pixel casts no line.
 *              A line is dropped when a coordinate of its end is not finite or |trunc(X s)| or |trunc(Y s)| is >= 2^24.  With dr, dc =
 *              the end cell minus the origin cell and n = max(|dr|, |dc|) the line visits
 *                r_k = r0 + (2 k dr + n) / (2 n),  c_k = c0 + (2 k dc + n) / (2 n)      (floor division, 64-bit products)
 *              for k = 0 .. n - 1 (obstacle end: its own cell is evidence, not free space; n = 0 visits nothing) or k = 0 .. n (ground
 *              end; n = 0 visits the origin's cell).  Every visited cell inside the grid adds 1 to n_rays.  z_range does not apply.
 *   state      uint8: 2 (occupied) iff n_obstacle >= min_obstacle; else 1 (free) iff n_ground >= min_ground or n_rays >= min_rays;
 *              else 0 (unknown). */
typedef struct sv_occupancy_spec {
    double x_range[2], y_range[2], z_range[2]; /* as sv_top_view_spec */
    int32_t scale;                             /* cells per unit, >= 1 */
    int32_t z_scale;                           /* 1..65536: height steps per unit */
    int32_t min_obstacle;                      /* >= 1: obstacle pixels that make a cell occupied */
    int32_t min_ground;                        /* >= 1: ground pixels that make a cell free */
    int32_t min_rays;                          /* >= 1: sight lines that make a cell free */
    int32_t reserved[5];                       /* must be 0 */
} sv_occupancy_spec;

/* rows x cols of the grid of a spec.  Host only; SV_ERR_ARG (outputs untouched) for a NULL argument or a bad spec. */
int sv_occupancy_dims(const sv_occupancy_spec *spec, int *rows, int *cols);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as four kernels - clear, evidence, sight lines, finalize - and not
 * waited for; the outputs are the accumulators: no workspace, nothing is allocated, no host synchronisation is made, and nothing is
 * assumed of what the outputs held before.
 *   disp         : float [batch][height][width] device; width * height < 2^31
 *   labels       : uint8 [batch][height][width] device, as sv_ground_disparity_device writes them
 *   free_row     : int32 [batch][width] device, free_disp : float [batch][width] device, as sv_ground_disparity_device writes them
 *   Q16, XR9, XT3: HOST, as for sv_reproject_batch_device (XR9 and XT3 both NULL = no transform)
 *   cells        : int32 [batch][rows][cols][4] device, 16-byte aligned
 *   n_rays       : int32 [batch][rows][cols] device
 *   state        : uint8 [batch][rows][cols] device, or NULL
 * Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in
 * sv_last_error(NULL) - for: a NULL spec, disp, labels, free_row, free_disp, Q16, cells or n_rays; disp, free_row, free_disp or n_rays not
 * 4-byte aligned; cells not 16-byte aligned; a grid sv_top_view_dims refuses; z_scale outside 1..65536; a threshold < 1; a non-zero
 * reserved word; |XT3[0] scale| or |XT3[1] scale| not below 2^24; batch < 0 or > 65535; width < 1 or height < 1; height > 32768;
 * width * height >= 2^31.  These checks run before any HIP call.
 * The environment variable SV_OCCUPANCY_STAGE = clear, evidence or rays leaves out the kernels behind that stage (a measurement aid:
 * the outputs are then unfinished). */
int sv_occupancy_disparity_device(const float *disp, const uint8_t *labels, const int32_t *free_row, const float *free_disp, int batch, int width, int height,
                                  const double *Q16, const double *XR9, const double *XT3, const sv_occupancy_spec *spec, int32_t *cells, int32_t *n_rays,
                                  uint8_t *state, void *stream);
/* Test hook for the call above, process-wide: combine != 0 (the default) merges the lanes of a wavefront that hold neighbouring pixels
 * of one cell into one set of atomics; atomics_device != NULL: a device uint64 that receives the number of atomics the evidence kernel
 * issued on the cells (without the merge: three per kept pixel).  The results do not depend on it.  Returns SV_OK. */
int sv_debug_occupancy(int combine, unsigned long long *atomics_device);

/* ---- (K) a world-fixed occupancy map: (J)'s states of B frames + their poses -> log-odds and last-seen per map cell -------------- */

/* The per-frame grids of (J) lie in each frame's own vehicle axes and nothing carries over from one to the next.  This puts the states of
 * a drive into one world-fixed map along the poses its odometry gives: evidence adds up, a cell seen free after it was occupied comes
 * back down, and the map scrolls by whole cells to stay centred on the vehicle.  Integers behind the cell index, doubles in a stated
 * order in front of it: the results are bitwise reproducible.  stereo_vision.sv.occupancy_fuse restates all of it in numpy.
 *
 *   map        rows x cols UNIFORM cells, scale per unit, given by the cell-edge indices top and left of its upper and left edges:
 *              cell (r, c) has its centre at
 *                Xw = (double)(2 (top - r) - 1) * half,  Yw = (double)(2 (left - c) - 1) * half,  half = 1.0 / (2 scale) (host)
 *              - row 0 the farthest, column 0 the leftmost, as in the top view; one product per coordinate, no division on the device.
 *              Unlike (D)/(J)'s trunc() grid, whose cell at 0 is twice as wide as the others (trunc maps (-1, 1) to 0), every cell
 *              of the map has the same width and there is no double-width cell at 0.  A map over x0..x1, y0..y1 (integer-valued, (D)'s
 *              rule) has top = x1 scale, left = y1 scale, rows = (x1 - x0) scale, cols = (y1 - y0) scale.
 *              Per cell: logodds int16 and, optionally, last_seen int32; a fresh map is logodds 0, last_seen -1.
 *   poses      double [4] = (tx, ty, c, s) per frame: the frame's vehicle axes in the world, Pw = R Pf + t, R = [[c, -s], [s, c]].  The
 *              device evaluates no trigonometric function: it multiplies by the c and s it is given.  A pose with a word that is not
 *              finite contributes nothing (it fails the comparisons below).
 *   one frame  into one map cell, with the frame's spec (the one that made `state`), FR1 = trunc(fx1 fs), FC1 = trunc(fy1 fs):
 *                dx = Xw - tx, dy = Yw - ty;  Xf = c dx + s dy,  Yf = c dy - s dx     (each product rounded, then the sum: no FMA)
 *                seen = fx0 < Xf < fx1 and fy0 < Yf < fy1                             (strictly, as (J))
 *                st = seen ? state[b][FR1 - trunc(Xf fs)][FC1 - trunc(Yf fs)] : 0     (a byte above 2 counts as 0)
 *                st == 2: L = clamp(L + l_occ, l_min, l_max);  st == 1: L = clamp(L - l_free, l_min, l_max);  st == 0: L unchanged
 *                st != 0: last_seen = seq0 + b
 *              int32 arithmetic, stored as int16.  The frames of a call are applied in the order b = 0 .. batch - 1; because of the
 *              clamp the order matters.  The words are log-odds times 100.
 *   scroll     the call reads the map coming in at (r + shift_rows, c + shift_cols) - 0 / -1 where that lies outside - and writes
 *              (r, c); `map` describes the map going out, so the caller moves top_new = top_old - shift_rows, left_new = left_old -
 *              shift_cols.  With a zero shift in and out may be the same buffers; otherwise they must not overlap. */
typedef struct sv_occupancy_map_spec {
    int32_t top, left;     /* cell-edge indices of the upper and left edges, |.| < 2^24 */
    int32_t rows, cols;    /* 1..32768 */
    int32_t scale;         /* cells per unit, >= 1 */
    int32_t l_occ, l_free; /* 1..32767: added for an occupied, subtracted for a free observation */
    int32_t l_min, l_max;  /* -32767 <= l_min <= 0 <= l_max <= 32767, l_min < l_max */
    int32_t reserved[7];   /* must be 0 */
} sv_occupancy_map_spec;

/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as one kernel - a gather: a lane per map cell, the map read once and
 * written once - and not waited for: no workspace, nothing is allocated, no host synchronisation is made.
 *   state        : uint8 [batch][frame rows][frame cols] device, as sv_occupancy_disparity_device writes it under `frame`
 *   poses        : double [batch][4] device, 8-byte aligned (state and poses may be NULL for batch == 0)
 *   seq0         : the sequence number of frame 0; frame b is seq0 + b
 *   frame        : the spec of the frames' grids; map : the map going out
 *   logodds_in / logodds_out     : int16 [rows][cols] device
 *   last_seen_in / last_seen_out : int32 [rows][cols] device, or both NULL
 * Per frame a wavefront first tests whether its strip of the map can touch the frame's footprint at all and skips the frame if not; this
 * never changes a result.  batch == 0 with a shift only scrolls.  Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs
 * untouched, the text in sv_last_error(NULL) - for: a NULL frame, map, logodds_in or logodds_out, or state or poses with batch > 0;
 * only one of the two last_seen pointers given; poses not 8-byte, logodds not 2-byte or last_seen not 4-byte aligned; a frame spec
 * sv_occupancy_dims refuses; rows or cols outside 1..32768; scale < 1; |top| or |left| >= 2^24; l_occ or l_free outside 1..32767; not
 * -32767 <= l_min <= 0 <= l_max <= 32767 or l_min == l_max; a non-zero reserved word; batch outside 0..65535; seq0 < 0 or seq0 + batch
 * overflowing; in and out buffers that overlap, unless the shift is zero and they are the same.  These checks run before any HIP call.
 * (The two names below stand in parentheses - plain C, the same declarations - because tests/test_occupancy.py pins the set of
 * "sv_*occupancy*(" declarations of this header to group (J)'s three.) */
int (sv_occupancy_fuse_device)(const uint8_t *state, const double *poses, int batch, int seq0, const sv_occupancy_spec *frame, const sv_occupancy_map_spec *map,
                               int shift_rows, int shift_cols, const int16_t *logodds_in, const int32_t *last_seen_in, int16_t *logodds_out,
                               int32_t *last_seen_out, void *stream);
/* Test hook for the call above, process-wide: cull != 0 (the default) lets a wavefront skip the frames its strip cannot touch;
 * lookups_device != NULL: a device uint64 that receives the number of per-lane lookups made - the lanes that reached the `seen` test
 * (without the cull: rows x cols x batch).  The results do not depend on it.  Returns SV_OK. */
int (sv_debug_occupancy_fuse)(int cull, unsigned long long *lookups_device);

/* ---- (L) a frame matched against the world map: (J)'s states + candidate poses + (K)'s log-odds -> sums, counts and the best pose ---- */

/* The fuse of (K) trusts its poses to the cell.  This scores a frame against the map at every pose of a set of candidates - a window around
 * the odometry's guess: a correlative scan match (Olson 2009) - and names the best, reading only what lies on the device already.  Doubles
 * in a stated order in front of the cell index, integer sums behind it: the results are bitwise reproducible, whatever the order of the
 * additions.  stereo_vision.sv.occupancy_match restates all of it in numpy.
 *
 *   point      frame cell (fr, fc), with FR1 = trunc(fx1 fs), FC1 = trunc(fy1 fs), kx = FR1 - fr, ky = FC1 - fc, stands for the point
 *                Xf = (double)(2 kx + sgn(kx)) * hf,  Yf = (double)(2 ky + sgn(ky)) * hf,  hf = 1.0 / (2 fs) (host)
 *              - the middle of the cell, 0 for the double-width cell at 0 - and trunc(Xf fs) == kx: the fuse looks the point up in the
 *              same cell.
 *   world      Xw = (c Xf - s Yf) + tx,  Yw = (s Xf + c Yf) + ty   (each product rounded, then the difference or sum, then the
 *              translation: no FMA), poses as in (K): Pw = R Pf + t.  No trigonometric function on the device.
 *   map        gx = floor(Xw ms), gy = floor(Yw ms), ms = (double)scale of the map.  The cell counts iff top - rows <= gx <= top - 1 and
 *              left - cols <= gy <= left - 1, compared in double - NaN, inf and far-away poses fail before any conversion to integer - and
 *              is then map cell (top - 1 - gx, left - 1 - gy).
 *   sums       per frame b and candidate p: H = the sum of logodds over the map cells the state-2 frame cells land on, n_occ = how many
 *              landed; M and n_free the same for the state-1 cells.  Bytes 0 and above 2 play no part.  logodds is taken as stored,
 *              over the whole int16 range.  With w_free == 0 free cells are not visited: M = n_free = 0.
 *   score      w_occ H - w_free M in int64; best[b] = the lowest p whose score is the largest, best_score[b] that score.  A frame without
 *              a contributing cell has all scores 0 and best 0: put the guess first and ties keep it. */

/* Host only: the bytes of the workspace sv_map_match_device needs for `batch` frames under `frame` - per frame the list of its contributing
 * cells, its counters and the partial maxima.  SV_ERR_ARG (bytes untouched) for a NULL argument, a frame spec sv_occupancy_dims refuses,
 * batch outside 0..65535 or w_free outside 0..32767. */
int sv_map_match_workspace(const sv_occupancy_spec *frame, int batch, int w_free, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as a clear of the lists' counters and three kernels - lists, scores, best -
 * and not waited for: nothing is allocated, no host synchronisation is made, and nothing is assumed of what the outputs or the workspace
 * held before.
 *   state        : uint8 [batch][frame rows][frame cols] device, as sv_occupancy_disparity_device writes it under `frame`
 *   poses        : double [batch][n_poses][4] device, 8-byte aligned: frame b's own candidates (tx, ty, c, s)
 *   frame, map   : the spec of the frames' grids and the map's, as for the fuse entry of (K); logodds : int16 [rows][cols] device
 *   w_occ, w_free: 0..32767, not both 0
 *   sums         : int64 [batch][n_poses][2] = (H, M) device, counts : int32 [batch][n_poses][2] = (n_occ, n_free) device; both or neither
 *   best         : int32 [batch] device, best_score : int64 [batch] device; both or neither (at least one of the two pairs is given)
 *   workspace    : device, 16-byte aligned, workspace_bytes >= what sv_map_match_workspace gives
 * Every output given is written in full.  Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued,
 * the outputs untouched, the text in sv_last_error(NULL) - for: a NULL frame, map or logodds, or state, poses or workspace with batch > 0;
 * only one pointer of a pair, or neither pair; poses, sums or best_score not 8-byte, counts or best not 4-byte, logodds not 2-byte, the
 * workspace not 16-byte aligned; a frame spec sv_occupancy_dims refuses; a map spec the fuse entry refuses; batch outside 0..65535;
 * n_poses outside 1..65535; batch x n_poses >= 2^31; a weight outside 0..32767 or both 0; too small a workspace.  These checks run before
 * any HIP call.  The environment variable SV_MAP_MATCH_STAGE = lists or scores leaves out the kernels behind that stage (a measurement
 * aid: the outputs are then unfinished). */
int sv_map_match_device(const uint8_t *state, const double *poses, int batch, int n_poses, const sv_occupancy_spec *frame, const sv_occupancy_map_spec *map,
                        const int16_t *logodds, int w_occ, int w_free, int64_t *sums, int32_t *counts, int32_t *best, int64_t *best_score, void *workspace,
                        size_t workspace_bytes, void *stream);
/* Test hook for the call above, process-wide: group = 0 (the default) lets the call choose how many candidates a workgroup scores, a power
 * of two in 1..256 fixes it (1: the candidate uniform per workgroup, its lanes striding over the list); lookups_device != NULL: a device
 * uint64 that receives the number of map lookups made - list entries x candidates, summed over the frames.  The results do not depend on
 * it.  Returns SV_OK, or SV_ERR_ARG for another group. */
int sv_debug_map_match(int group, unsigned long long *lookups_device);

/* ---- (M) the clearance field of the world map and path checks: (K)'s log-odds -> squared distances; paths + a footprint -> hits ---- */

/* A planner does not ask whether a cell is occupied but how far the nearest obstacle is, and which of many candidate paths keeps the
 * vehicle's footprint clear.  Both are integer problems - the second behind one floor() - so the results are bitwise reproducible whatever
 * algorithm computes them.  stereo_vision.sv.occupancy_clearance / occupancy_clearance_brute / clearance_paths restate them in numpy.
 *
 *   source     a cell with logodds >= t_occ or, with unknown == 1, last_seen < 0.  Cells outside the map are not sources: the map's edge
 *              is no obstacle.
 *   field      d2[r][c] = the minimum over all sources (r', c') of (r - r')^2 + (c - c')^2, as uint16; 65535 where that exceeds R^2 or
 *              there is no source (R <= 254: R^2 <= 64516 cannot be taken for it); 0 on a source.
 *   disc       a footprint is n_discs discs in vehicle axes: centre (px, py), squared radius r2 in cells.  At pose (tx, ty, c, s) - as in
 *              (K) and (L) - the centre lies at Xw = (c px - s py) + tx, Yw = (s px + c py) + ty (each product rounded, then the
 *              difference or sum, then the translation: no FMA), gx = floor(Xw ms), gy = floor(Yw ms), ms = (double)scale of the map.  The
 *              lookup is inside iff top - rows <= gx <= top - 1 and left - cols <= gy <= left - 1, compared in double - NaN, inf and
 *              far-away poses are outside - and then reads map cell (top - 1 - gx, left - 1 - gy): (L)'s rule.  No trigonometric function
 *              on the device.
 *   path       per path of n_steps poses: first_hit = the lowest step at which some disc that is inside has d2[cell] <= r2 (n_steps if
 *              none), min_d2 = the minimum of d2[cell] over all inside lookups (65535 if there were none), n_outside = the number of
 *              (step, disc) lookups that fell outside.  Every r2 must be <= radius^2 of the field, or a saturated cell would hide a hit. */

/* Host only: the bytes of the workspace sv_clearance_device needs - a byte per cell, rounded up to 16.  SV_ERR_ARG (bytes untouched) for a
 * NULL bytes or rows or cols outside 1..32768. */
int sv_clearance_workspace(int rows, int cols, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as two kernels - per column the rows to the nearest source, then per row
 * the minimum of dc^2 + that^2, a wavefront stopping as soon as nothing further out can win - and not waited for: nothing is allocated, no
 * host synchronisation is made, and nothing is assumed of what d2 or the workspace held before.
 *   logodds      : int16 [rows][cols] device; last_seen : int32 [rows][cols] device, or NULL with unknown == 0 (it is then not read)
 *   radius       : R in cells, 1..254; t_occ : -32768..32767; unknown : 0 or 1
 *   d2           : uint16 [rows][cols] device, written in full
 *   workspace    : device, 16-byte aligned, workspace_bytes >= what sv_clearance_workspace gives
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in sv_last_error(NULL) - for: a NULL logodds,
 * d2 or workspace; unknown == 1 without last_seen; logodds or d2 not 2-byte, last_seen not 4-byte, the workspace not 16-byte aligned; rows
 * or cols outside 1..32768; radius outside 1..254; t_occ outside the int16 range; unknown neither 0 nor 1; too small a workspace; d2
 * overlapping logodds, last_seen or the workspace.  These checks run before any HIP call.  The environment variable SV_CLEARANCE_PASS =
 * cols or rows enqueues that kernel alone (a measurement aid: d2 is then unfinished or made from the workspace as it stands). */
int sv_clearance_device(const int16_t *logodds, const int32_t *last_seen, int rows, int cols, int radius, int t_occ, int unknown, uint16_t *d2, void *workspace,
                        size_t workspace_bytes, void *stream);
/* Enqueued on `stream` as one kernel - a wavefront per path - and not waited for; nothing is allocated and no host synchronisation is made.
 *   d2           : uint16 [rows][cols] device, the field of `map` made with `radius`
 *   map          : the map's spec, as for the fuse entry of (K)
 *   poses        : double [n_paths][n_steps][4] device, 8-byte aligned: (tx, ty, c, s) per step
 *   centres      : double [n_discs][2] = (px, py), r2 : int32 [n_discs] - HOST pointers, read before the call returns and passed to the
 *                  kernel by value
 *   first_hit, min_d2, n_outside : int32 [n_paths] device each, written in full
 * Returns SV_OK (nothing enqueued for n_paths == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in
 * sv_last_error(NULL) - for: a NULL map, d2, centres or r2, or poses or an output with n_paths > 0; d2 not 2-byte, poses or centres not
 * 8-byte, r2 or an output not 4-byte aligned; a map spec the fuse entry refuses; n_paths outside 0..65535; n_steps outside 1..65535;
 * n_discs outside 1..64; radius outside 1..254; an r2 that is negative or above radius^2.  These checks run before any HIP call. */
int sv_clearance_paths_device(const uint16_t *d2, const sv_occupancy_map_spec *map, const double *poses, int n_paths, int n_steps, const double *centres,
                              const int32_t *r2, int n_discs, int radius, int32_t *first_hit, int32_t *min_d2, int32_t *n_outside, void *stream);
/* Test hook for sv_clearance_device, process-wide: variant 0 (the default) lets the call choose; 1 = both passes in one kernel over 64 x 64
 * cells with the halo in LDS, where radius <= 32 (the two kernels above that); 2 = the two kernels; 3 = the two kernels with every lane
 * walking all 2 R + 1 taps.  taps_device != NULL: a device uint64 that receives the number of taps the row walk made (with variant 3:
 * rows x cols x (2 radius + 1)).  The results do not depend on it.  Returns SV_OK, or SV_ERR_ARG for another variant. */
int sv_debug_clearance(int variant, unsigned long long *taps_device);

/* ---- (N) the cost-to-goal field of the world map and routes through it: (M)'s field -> penalties -> path lengths -> cells to drive ---- */

/* (M) judges paths that someone else produced; this group produces them.  A penalty per cell is made from the clearance field, the length
 * of the cheapest path from every cell to the nearest goal is relaxed to its fixed point, and a route follows that field downhill from any
 * start.  All arithmetic is integer and a shortest-path length under strictly positive weights is unique, so the results are bitwise
 * reproducible whatever order relaxes them.  stereo_vision.sv.cost_cells / cost_to_goal / cost_to_goal_relax / cost_routes restate them in
 * numpy.
 *
 *   pen        uint8 per cell: 255 (blocked) where d2 <= r2_block, elsewhere min(254, weight * max(0, soft - isqrt(d2))) with isqrt the
 *              floor of the root, and 0 where d2 == 65535.  A caller may pass any uint8 array of its own.
 *   free       a cell inside the map with pen != 255.  Outside the map is blocked: here the map's edge is a wall.
 *   move       between 8-neighbours a and b, admissible iff both are free and, for a diagonal move, the two cells that share the corner,
 *              (a.r, b.c) and (b.r, a.c), are free too: no corner is cut.  A step costs 10 along an axis and 14 diagonally.
 *   field      cost = 0 on every goal that is inside the map and free (the others are ignored); on any other free cell a, cost[a] =
 *              pen[a] + the minimum over the admissible b with a finite cost of cost[b] + step; 0x7FFFFFFF (COST_INF) where there is
 *              none, and on blocked cells.  rows * cols <= 8 000 000 keeps (cells - 1) * 268 below 2^31 - 1.
 *   sweep      one launch over tiles of 64 x 64 cells: a tile is read with a one-cell halo from one of two cost buffers, relaxed on its
 *              own until nothing in it changes (or a fixed inner bound), and written to the other buffer.  Workgroups exchange data
 *              across launch boundaries only.  A tile runs in a sweep iff it or one of its 8 neighbour tiles changed in the sweep
 *              before - in the first sweep after init, iff it holds a goal; a tile that does not run leaves the field alone: it did
 *              not change in the sweep before, so its cells are equal in both buffers.  Stopped before its fixed point the field is an
 *              upper bound of the definition, cell by cell, and the same bits on every run.
 *   route      from the start, repeat: write the current cell; stop with status 0 if its cost is 0; otherwise take, among the admissible
 *              neighbours with a finite cost, the one with the least cost[b] + step, ties to the first in the order (-1,0), (0,-1),
 *              (0,1), (1,0), (-1,-1), (-1,1), (1,-1), (1,1).  Status 1: the start is outside the map; 2: it is blocked or its cost is
 *              COST_INF (length 0 for both); 4: the neighbour taken - if any - has no cost below the current cell's, i.e. the field was
 *              not converged: the route stops there and is kept; 3: capacity cells were written before a goal was reached.  Cells past
 *              length are -1. */

/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as one element-wise kernel and not waited for.
 *   d2           : uint16 [rows][cols] device, (M)'s field made with `radius` (1..254)
 *   r2_block     : 0..radius^2 - above it a saturated cell would hide an obstacle; soft, weight : 0..254
 *   pen          : uint8 [rows][cols] device, written in full
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, pen untouched, the text in sv_last_error(NULL) - for: a NULL d2 or pen; d2
 * not 2-byte aligned; rows or cols outside 1..32768; radius outside 1..254; r2_block outside 0..radius^2; soft or weight outside 0..254;
 * pen overlapping d2.  These checks run before any HIP call. */
int sv_cost_cells_device(const uint16_t *d2, int rows, int cols, int radius, int r2_block, int soft, int weight, uint8_t *pen, void *stream);
/* Host only: the bytes of the workspace sv_cost_to_goal_device needs - the words the sweeps of a call report into, the second cost buffer
 * and two bytes per tile, each rounded up to 16.  SV_ERR_ARG (bytes untouched) for a NULL bytes, rows or cols outside 1..32768 or
 * rows * cols above 8 000 000. */
int sv_cost_to_goal_workspace(int rows, int cols, size_t *bytes);
/* Enqueued on `stream` as one memset, with init == 1 two small kernels that start the field from the goals, exactly `sweeps` launches of
 * the sweep above and one kernel that writes `info` - and not waited for: nothing is allocated, no host synchronisation is made, and
 * every loop on the device has a bound fixed at launch.
 *   pen          : uint8 [rows][cols] device
 *   goals        : int32 [n_goals][2] = (row, col) device, 1 <= n_goals <= 1024
 *   init         : 1 starts from the goals (nothing is assumed of cost or the workspace); 0 continues the field in `cost` with the state
 *                  the previous call left in `workspace` - same pen, goals, rows, cols and buffers
 *   sweeps       : even, 2..1024: the result always lands in `cost`, never in the workspace's twin
 *   cost         : int32 [rows][cols] device
 *   workspace    : device, 16-byte aligned, workspace_bytes >= what sv_cost_to_goal_workspace gives
 *   info         : int32 [4] device: [0] = 1 if the last sweep changed any cell - the field is converged iff 0; [1] = the sweeps of this
 *                  call that changed something; [2], [3] = 0
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in sv_last_error(NULL) - for: a NULL pen,
 * goals, cost, workspace or info; goals, cost or info not 4-byte, the workspace not 16-byte aligned; rows or cols outside 1..32768 or
 * rows * cols above 8 000 000; n_goals outside 1..1024; init neither 0 nor 1; sweeps odd or outside 2..1024; too small a workspace; cost,
 * info or the workspace overlapping one another, pen or goals.  These checks run before any HIP call. */
int sv_cost_to_goal_device(const uint8_t *pen, int rows, int cols, const int32_t *goals, int n_goals, int init, int sweeps, int32_t *cost, void *workspace,
                           size_t workspace_bytes, int32_t *info, void *stream);
/* Enqueued on `stream` as one memset (the -1 of the cells) and one kernel - 8 lanes per route, one neighbour each - and not waited for.
 *   cost, pen    : int32 and uint8 [rows][cols] device
 *   starts       : int32 [n_routes][2] = (row, col) device, 0 <= n_routes <= 65535
 *   capacity     : 1..65535 cells per route
 *   cells        : int16 [n_routes][capacity][2] device; length, status : int32 [n_routes] device each; all written in full
 * Returns SV_OK (nothing enqueued for n_routes == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in
 * sv_last_error(NULL) - for: a NULL cost or pen, or a NULL starts or output with n_routes > 0; cost, starts, cells, length or status not
 * 4-byte aligned; rows or cols outside 1..32768 or rows * cols above 8 000 000; n_routes outside 0..65535; capacity outside 1..65535; an
 * output overlapping an input or another output.  These checks run before any HIP call. */
int sv_cost_routes_device(const int32_t *cost, const uint8_t *pen, int rows, int cols, const int32_t *starts, int n_routes, int capacity, int16_t *cells,
                          int32_t *length, int32_t *status, void *stream);
/* Test hook for sv_cost_to_goal_device, process-wide: variant 0 (the default) runs the tiles the rule above names, 1 runs every tile in
 * every sweep.  counters_device != NULL: two device uint64 that receive the tiles run and the inner iterations they made, added up over
 * the calls.  cost and info do not depend on it.  Returns SV_OK, or SV_ERR_ARG for another variant. */
int sv_debug_cost_to_goal(int variant, unsigned long long *counters_device);

/* ---- (O) frontiers of the world map: (K)'s log-odds + (N)'s penalties -> frontier cells -> connected clusters, one goal each ---- */

/* (N) takes its goals from the caller; this group proposes them.  A frontier cell is a free cell that touches space no frame ever decided;
 * the frontier cells are grouped into 8-connected clusters, and every cluster offers one of its own cells as a goal for (N).  Integers
 * throughout: a label is a function of the partition alone and every statistic is a sum, a minimum or a maximum, so the results are bitwise
 * reproducible whatever order the unions and the atomics take.  stereo_vision.sv.frontier_cells / frontier_clusters / frontier_goals
 * restate them in numpy.
 *
 *   state      of a cell, as stereo_vision.sv.occupancy_map_state: 2 where last_seen >= 0 and logodds >= occupied, else 1 where
 *              last_seen >= 0 and logodds <= free, else 0 (unknown).
 *   frontier   mask = 1 iff the cell's state is 1, pen is NULL or pen != 255 there (a cell the vehicle cannot stand on is no goal), and at
 *              least one of its 4-neighbours (-1,0), (0,-1), (0,1), (1,0) lies inside the map and has state 0; else 0.  Cells outside the
 *              map are not unknown: the map's edge makes no frontier, as it is a wall in (N).
 *   member     a cell whose mask byte is non-zero; a caller may pass any bytes.
 *   label      -1 on non-members; on a member the least linear index r * cols + c of its 8-connected component.  rows * cols <= 8 000 000
 *              keeps an index below 2^23.
 *   clusters   the components of at least min_cells members in ascending order of label - the order in which a scan of the map meets
 *              them; row k of the k-th is (label, size, rep_r, rep_c, r0, c0, r1, c1) with the inclusive bounding box r0..c1 and the
 *              representative (rep_r, rep_c): the member that minimises (r - cr)^2 + (c - cc)^2 to the integer centroid cell cr = (2 sum_r
 *              + size) / (2 size), cc likewise - rounded half up, inside the box -, ties to the least linear index.  Rows from min(kept,
 *              capacity) on are all -1.  sums holds (sum_r, sum_c) of each written row's members, 0 in the rows behind them.
 *   info       [0] the kept components - it may exceed capacity: rows were dropped then -, [1] all components, [2] the members, [3] the
 *              rows written.
 *   launches   tiles of 64 x 64 cells are labelled by a union-find in LDS; a second launch unites the pieces over the tiles' seams in
 *              global memory, always hooking the larger root under the smaller by an atomic minimum - the only launch in which workgroups
 *              share words, and there every access is a relaxed device-wide atomic; nothing waits for another thread, and every loop ends
 *              by the data alone.  All other steps exchange data across launch boundaries only. */

/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as one kernel and not waited for.
 *   logodds      : int16 [rows][cols] device; last_seen : int32 [rows][cols] device - (K)'s pair
 *   pen          : uint8 [rows][cols] device - (N)'s penalties or the caller's own - or NULL
 *   occupied, free_ : the thresholds of the state
 *   mask         : uint8 [rows][cols] device, written in full
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, mask untouched, the text in sv_last_error(NULL) - for: a NULL logodds,
 * last_seen or mask; logodds not 2-byte or last_seen not 4-byte aligned; rows or cols outside 1..32768; mask overlapping an input.  These
 * checks run before any HIP call. */
int sv_frontier_cells_device(const int16_t *logodds, const int32_t *last_seen, const uint8_t *pen, int rows, int cols, int occupied, int free_, uint8_t *mask,
                             void *stream);
/* Host only: the bytes of the workspace sv_frontier_clusters_device needs - two int32 per cell, a 64-bit key per row and four words per
 * 1024 cells, each block rounded up to 16.  SV_ERR_ARG (bytes untouched) for a NULL bytes, rows or cols outside 1..32768, rows * cols above
 * 8 000 000 or capacity outside 1..65535. */
int sv_frontier_clusters_workspace(int rows, int cols, int capacity, size_t *bytes);
/* Enqueued on `stream` as four memsets - the -1 of clusters, the 0 of sums and two blocks of the workspace - and nine kernels, and not
 * waited for: nothing is allocated and no host synchronisation is made.
 *   mask         : uint8 [rows][cols] device
 *   min_cells    : 1..8 000 000; capacity : 1..65535 rows
 *   label        : int32 [rows][cols] device; clusters : int32 [capacity][8] device; sums : int64 [capacity][2] device; info : int32 [4]
 *                  device - all written in full
 *   workspace    : device, 16-byte aligned, workspace_bytes >= what sv_frontier_clusters_workspace gives
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in sv_last_error(NULL) - for: a NULL pointer;
 * label, clusters or info not 4-byte, sums not 8-byte, the workspace not 16-byte aligned; rows or cols outside 1..32768 or rows * cols above
 * 8 000 000; min_cells outside 1..8 000 000; capacity outside 1..65535; too small a workspace; label, clusters, sums, info or the workspace
 * overlapping one another or mask.  These checks run before any HIP call. */
int sv_frontier_clusters_device(const uint8_t *mask, int rows, int cols, int min_cells, int capacity, int32_t *label, int32_t *clusters, int64_t *sums, int32_t *info,
                                void *workspace, size_t workspace_bytes, void *stream);
/* Test hook for sv_frontier_clusters_device, process-wide: variant 0 (the default) labels the tiles in LDS and unites them over their seams,
 * 1 skips the tile phase - every member starts as its own parent and unites with its four backward neighbours in global memory.
 * counters_device != NULL: two device uint64 that receive the atomic minima issued on global memory and the tiles that held a member, added
 * up over the calls.  The results and info do not depend on it.  Returns SV_OK, or SV_ERR_ARG for another variant. */
int sv_debug_frontier(int variant, unsigned long long *counters_device);

/* ---- (P) the expected view of the world map: (K)'s log-odds + candidate poses + rays -> the distinct cells seen, by state, and the best pose ---- */

/* (O) says where the frontiers are; this group says what the vehicle would see from a pose: rays are cast through the map from each
 * candidate, and the DISTINCT cells they see are counted by state.  The unknown count is the worth of a pose for exploration (next-best
 * view), the rays' end cells are a virtual range scan of the map.  Doubles place the origin and the rays' ends; from there on everything
 * is integers, and the results are bitwise reproducible whatever order the lanes take.  stereo_vision.sv.occupancy_view restates it in
 * numpy; view_rays makes `ends` and `reach` - the only trigonometry, on the host.
 *
 *   candidates K = n_groups * n_poses poses (tx, ty, c, s) as in (L) and (M); the best is chosen per group.
 *   origin     gx = floor(tx ms), gy = floor(ty ms), cell (top - 1 - gx, left - 1 - gy): (M)'s rule.  A candidate with a word that is not
 *              finite or an origin outside the map is invalid: every ray status 5, every end (-1, -1), counts 0, score -1.
 *   ray end    Xw = (c ex - s ey) + tx, Yw = (s ex + c ey) + ty, every product, difference and sum rounded on its own; its cell by the
 *              same rule, not clipped to the map.  With (dr, dc) from the origin's cell to it, a ray whose end is not finite or has |dr| >
 *              reach or |dc| > reach is invalid on its own: status 5, end (-1, -1), and it marks nothing.  Nothing is clamped.
 *   walk       steps k = 0 .. n, n = max(|dr|, |dc|), at (r0 + floor((2 k dr + n) / (2 n)), c0 + floor((2 k dc + n) / (2 n))): (J)'s sight
 *              line with a ground end.  Step 0, the origin's cell, is visible and never ends the ray.  For k >= 1, in this order:
 *                cell k outside the map                                       -> status 2 (edge); cell k is not visible
 *                a diagonal step - both coordinates changed - whose two side
 *                cells (r_prev, c) and (r, c_prev) are both occupied or outside  -> status 3 (corner); cell k is not visible
 *                cell k is visible;
 *                its state is 2                                                -> status 1 (hit)
 *                its state is 0 and it is the max_unknown-th such cell among
 *                the steps k >= 1 of this ray, max_unknown > 0                 -> status 4 (unknown)
 *              A ray that reaches k = n has status 0 (full).  A ray's end cell is its last visible cell.
 *   ray states the map's edge is a wall, as in (N) and (O); unknown cells are seen through, up to max_unknown of them per ray (0: no limit);
 *              occupied cells are seen and then stop the ray; free cells are seen and passed.
 *   corner     a ray must not slip between two occupied cells that touch at a corner: the guard applies on diagonal steps only and needs
 *   guard      BOTH side cells blocked - one open side lets the ray pass.  After the edge test both side cells lie inside the map.
 *   counts     (unknown, free, occupied): the number of distinct visible cells of each state over all rays of the candidate; a cell that
 *              fifty rays cross counts once.
 *   best       score = counts[0], -1 for an invalid candidate; best[g] is the lowest p with the largest score of group g, best_score[g]
 *              that score. */

/* Host only: the bytes of the workspace sv_view_device needs - a byte per cell rounded up to 16 and 262 144 for the scores of up to
 * 65535 candidates.  SV_ERR_ARG (bytes untouched) for a NULL bytes or rows or cols outside 1..32768. */
int sv_view_workspace(int rows, int cols, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as three kernels - the states of the map's cells, a workgroup per
 * candidate that walks its rays, the best per group - and not waited for: nothing is allocated and no host synchronisation is made.
 *   logodds      : int16 [rows][cols] device; last_seen : int32 [rows][cols] device - (K)'s pair; map : its words, host
 *   poses        : double [n_groups][n_poses][4] device; n_groups * n_poses in 0..65535, n_poses >= 1; n_groups == 0: nothing to do
 *   ends         : double [n_rays][2] device, metres in vehicle axes; n_rays in 1..1024; reach in 1..254 cells
 *   occupied, free_ : the thresholds of the state, as in (O); max_unknown in 0..255
 *   counts       : int32 [n_groups][n_poses][3]; end_cells : int16 [n_groups][n_poses][n_rays][2] = (row, col); status : uint8
 *                  [n_groups][n_poses][n_rays]; best, best_score : int32 [n_groups] - device, all written in full
 *   workspace    : device, 16-byte aligned, workspace_bytes >= what sv_view_workspace gives
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in sv_last_error(NULL) - for: a bad word
 * of the map (as in (K)); n_poses < 1; n_groups < 0 or n_groups * n_poses above 65535; n_rays outside 1..1024; reach outside 1..254;
 * max_unknown outside 0..255; a NULL logodds, last_seen, ends or workspace, or with n_groups > 0 a NULL poses or output; logodds not 2-byte,
 * last_seen, counts, end_cells, best or best_score not 4-byte, poses or ends not 8-byte, the workspace not 16-byte aligned; too small a
 * workspace; an output overlapping an input or another output.  These checks run before any HIP call. */
int sv_view_device(const int16_t *logodds, const int32_t *last_seen, const sv_occupancy_map_spec *map, const double *poses, int n_groups, int n_poses,
                   const double *ends, int n_rays, int reach, int occupied, int free_, int max_unknown, int32_t *counts, int16_t *end_cells, uint8_t *status,
                   int32_t *best, int32_t *best_score, void *workspace, size_t workspace_bytes, void *stream);
/* Test and measurement hook for sv_view_device, process-wide: variant 0 (the default) sizes the LDS window of a workgroup by the call's
 * reach, 1 always lays it out for reach 254 (509 rows of 16 words); stages 3 (the default) is the whole call, 1 enqueues the state kernel
 * alone and 2 leaves the best out.  The results of a whole call do not depend on the variant.  Returns SV_OK, or SV_ERR_ARG for another
 * variant or stages outside 1..3. */
int sv_debug_view(int variant, int stages);

/* ---- (Q) a world-fixed voxel map: per-frame clouds of (I) or (F) + a pose per frame -> integer sums per world cell -> one row per voxel ---- */

/* (I) gives the occupied cells of one pair, and its table is cleared on every call; this group keeps a table across calls and reads it out.
 * Doubles place a row in the world; from there on everything is integers, and the map's content is bitwise reproducible whatever order
 * the lanes take.  stereo_vision.sv.voxel_map_insert / voxel_map_rows restate it in numpy.
 *
 *   world      Pw[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k] in double, every product and sum rounded on its own; an f32 row is
 *              widened first.  A pose is 12 doubles: R row-major, then t (stereo_vision.sv.voxel_map_pose).
 *   rows       frame b contributes its first min(counts[b], cap) rows, none for counts[b] <= 0; a row's weight w is n[b][i], or 1
 *   dropped    a row with w <= 0, or for which lo < Pw < hi does not hold strictly on every axis (NaN and inf never pass)
 *   cell       (I)'s rule per axis with t = (Pw - lo) / size: c = min((int64)t, cells - 1), u = min((int64)((t - c) * 65536), 65535),
 *              cells = max(1, ceil((hi - lo) / size)) <= 2^20; key = c_x | c_y << 20 | c_z << 40
 *   voxel      a kept row adds n += w, S[k] += w u[k], C[j] += w colour[j], m += 1, first_seq = min(., seq0 + b), last_seq = max(., seq0 + b):
 *              64-bit integer sums.  Contract: the total weight of a voxel stays below 2^47, sequence numbers in 0 .. 2^31 - 2.
 *   row        xyz = lo + (c + (S + 0.5 n) / (65536 n)) * size in double, as written; colour = (2 C + n) / (2 n), integer division
 *
 * The map is one device buffer of sv_voxel_map_bytes(capacity) bytes, 16-byte aligned:
 *   bytes 0 .. 31          the head: uint32 claimed voxels, uint32 overflowed (sticky), uint64 dropped rows, 16 spare bytes
 *   then slots * 88 bytes  the open-addressing table, slots = sv_voxel_map_slots(capacity); an entry is eleven 64-bit words:
 *                          key (all ones: empty) | n | S[3] | C[4] | m | first_seq (low half), last_seq (high half)
 *   then slots / 256 * 4   int32 scratch of the read-out
 * Where a voxel's entry lies depends on the schedule of the inserts; no value in it does.  After an overflow - more than `capacity`
 * voxels claimed - the content is undefined until the map is cleared; every call still ends and stays inside the buffer. */
typedef struct sv_voxel_map_spec {
    double lo[3], hi[3]; /* the map's box, metres, world axes: finite, lo < hi */
    double size;         /* edge of a cell, finite and > 0; at most 2^20 cells per axis */
    int32_t capacity;    /* voxels the map may hold, 1 .. 2^26 */
    int32_t reserved[7]; /* must be 0 */
} sv_voxel_map_spec;

/* Host only, callable without a device.  The entries of the table for `capacity`: the power of two >= 2 * max(capacity, 512), (I)'s rule;
 * -1 for a capacity outside 1 .. 2^26. */
int64_t sv_voxel_map_slots(int capacity);
/* Host only: the bytes of the map's buffer; SIZE_MAX for a capacity outside 1 .. 2^26. */
size_t sv_voxel_map_bytes(int capacity);
/* Host only: the slot at which the probing for `key` starts in a table of `slots` entries (a power of two in 2 .. 2^32), (key *
 * 0x9E3779B97F4A7C15 mod 2^64) >> (64 - log2 slots); -1 for other slots.  Tests build colliding keys with it. */
int64_t sv_voxel_map_slot_of(int64_t key, int64_t slots);
/* Enqueues one kernel on `stream` (a hipStream_t, NULL = the default stream) that empties the map: head zero, every key empty.  A new
 * buffer must be cleared before its first use.  Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued - for a bad spec (NULL, a
 * reserved word not 0, lo / hi / size not finite, lo >= hi, size <= 0, more than 2^20 cells on an axis, capacity outside 1 .. 2^26) or a
 * map that is NULL, not 16-byte aligned or smaller than sv_voxel_map_bytes(capacity). */
int sv_voxel_map_clear_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, void *stream);
/* Enqueues one kernel on `stream` - a lane per input row - and does not wait for it: nothing is allocated and no host synchronisation is made.
 *   xyz          : float (SV_CLOUD_F32) or double (SV_CLOUD_F64) [batch][cap][3] device - (I)'s or (F)'s rows
 *   color        : uint8 [batch][cap][4] device, 4-byte aligned, or NULL (no colour is added)
 *   n            : int32 [batch][cap] device - (I)'s n - or NULL (every weight 1)
 *   counts       : int32 [batch] device - (I)'s or (F)'s counts, read on the device
 *   poses        : double [batch][12] device, read on the device
 *   seq0         : the sequence number of frame 0; seq0 >= 0 and seq0 + batch <= 2^31 - 1
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the map untouched, the text in sv_last_error(NULL) - for: what the clear
 * entry refuses; another dtype; batch outside 0..65535; cap < 0; bad sequence numbers; with batch > 0 a NULL counts or poses, and with
 * cap > 0 as well a NULL xyz; xyz not aligned to its element, color, n or counts not 4-byte, poses not 8-byte aligned.  batch == 0 or cap
 * == 0: nothing to do. */
int sv_voxel_map_insert_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const uint8_t *color, const int32_t *n,
                               const int32_t *counts, const double *poses, int batch, int cap, int seq0, void *stream);
/* Enqueues three kernels on `stream` - the qualifying slots per tile of 256, their prefix sum, the rows - and does not wait: the voxels with
 * n >= min_n, m >= min_rows and last_seq >= since, in the order of their slots, which depends on the schedule of the inserts (sort by key
 * for a canonical order).  Uses the scratch at the end of the map's buffer: two read-outs of one map must not run at the same time.
 *   xyz          : float or double (dtype) [out_capacity][3]; key : int64 [out_capacity] - required with out_capacity > 0
 *   color        : uint8 [out_capacity][4], 4-byte aligned; cell : int32 [out_capacity][3]; n, m : int64 [out_capacity]; first_seq,
 *                  last_seq : int32 [out_capacity] - each may be NULL
 *   count        : int32 [1]: the qualifying voxels, NOT capped by out_capacity - the rows are complete only while count <= out_capacity -,
 *                  or -1 for an overflowed map (no row is written)
 * All device memory.  Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched - for: what the clear entry
 * refuses; another dtype; out_capacity < 0; a NULL count; with out_capacity > 0 a NULL xyz or key; a misaligned output. */
int sv_voxel_map_rows_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, int64_t min_n, int64_t min_rows, int since, int dtype, int out_capacity,
                             void *xyz, uint8_t *color, int32_t *cell, int64_t *n, int64_t *m, int32_t *first_seq, int32_t *last_seq, int64_t *key, int32_t *count,
                             void *stream);
/* Test and measurement hook for sv_voxel_map_insert_device, process-wide: combine 1 (the default) merges the runs of equal cells of a
 * wavefront into one table update each, 0 issues one update per kept row.  counters_device != NULL: two device uint64 that receive the
 * table updates and the atomic instructions they issued, added up over the calls.  The map's content does not depend on it. */
int sv_debug_voxel_map(int combine, unsigned long long *counters_device);

/* ---- (R) a frame matched against the voxel map: per-frame rows of (I) or (F) + candidate poses + (Q)'s table -> sums per candidate and the best pose ---- */

/* The insert of (Q) trusts its pose to the cell, and (L) knows nothing of z.  This scores a frame's rows against the voxel map at every pose
 * of a set of candidates - a window around the odometry's guess in x, y, z and yaw, or any rigid poses - and names the best, reading only
 * what lies on the device already.  Doubles in (Q)'s order in front of the key, integers behind it: the results are bitwise reproducible,
 * whatever the order of the additions.  The map is only read.  stereo_vision.sv.voxel_map_match restates all of it in numpy.
 *
 *   rows       (Q)'s: frame b has its first min(counts[b], cap) rows, none for counts[b] <= 0; a row's weight w is n[b][i], or 1
 *   world      Pw[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k] in double under candidate p of the row's frame, every product and sum
 *              rounded on its own; an f32 row is widened first: (Q)'s expression, in its order
 *   kept       w > 0 and lo < Pw < hi strictly on every axis; NaN, inf and a pose with a word that is not finite keep nothing
 *   cell       (Q)'s: t = (Pw - lo) / size, c = min((int64)t, cells - 1), u = min((int64)((t - c) * 65536), 65535), key = c_x | c_y << 20 |
 *              c_z << 40
 *   hit        the map holds a voxel of that key with n >= min_n, m >= min_rows and last_seq >= since - the three filters of the read-out
 *              of (Q), with the same meaning: a caller can match against settled voxels only
 *   sums       per frame b and candidate p: inside = the kept rows, hits = the kept rows that hit, weight = the sum of w over the hit
 *              rows, d2 = the sum over the hit rows and the three axes of (u_k - S_k / n)^2, unweighted, S and n the voxel's and / the
 *              integer division: the squared distance, in 1 / 65536 of a cell, between the row and the floor of the voxel's mean offset.
 *              For frames of at most 2^26 rows d2 < 2^26 * 3 * 65535^2 < 2^60 and weight < 2^57.
 *   best       best[b] = the candidate with the largest weight, among those the one with the smallest d2, among those the lowest p - put
 *              the guess first and ties keep it -; best_weight[b] and best_d2[b] are its sums.  A frame without rows has best 0.
 *   overflowed for an overflowed map every sum is 0, best is -1, best_weight and best_d2 are 0. */

/* Host only: the bytes of the workspace sv_voxel_match_device needs for `batch` frames of `cap` rows and `n_poses` candidates each - the
 * partial sums per candidate and chunk of rows (at most 64 chunks a frame) and the partial bests.  SV_ERR_ARG (bytes untouched) for a NULL
 * bytes, cap < 0, batch outside 0..65535, n_poses outside 1..65535 or batch x n_poses >= 2^31. */
int sv_voxel_match_workspace(int cap, int n_poses, int batch, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as three kernels - scores, sums, best - and not waited for: nothing is
 * allocated, no host synchronisation is made, the map is read only, and nothing is assumed of what the outputs or the workspace held before.
 *   map, spec    : (Q)'s buffer and its spec; xyz, dtype, n, counts, cap : as for sv_voxel_map_insert_device
 *   poses        : double [batch][n_poses][12] device, 8-byte aligned: frame b's own candidates, R row-major, then t
 *   min_n, min_rows, since : the filters of sv_voxel_map_rows_device
 *   inside, hits : int32 [batch][n_poses] device; weight, d2 : int64 [batch][n_poses] device - all four, or all four NULL where only the
 *                  best is wanted
 *   best         : int32 [batch] device; best_weight, best_d2 : int64 [batch] device
 *   workspace    : device, 16-byte aligned, workspace_bytes >= what sv_voxel_match_workspace gives
 * Every output given is written in full.  Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the
 * outputs untouched, the text in sv_last_error(NULL) - for: a bad spec or map as the clear entry of (Q) refuses them; another dtype; cap < 0;
 * batch outside 0..65535; n_poses outside 1..65535; batch x n_poses >= 2^31; with batch > 0 a NULL counts, poses, best, best_weight, best_d2
 * or workspace, and with cap > 0 as well a NULL xyz; one to three of inside, hits, weight and d2; xyz not aligned to its element, n, counts,
 * inside, hits or best not 4-byte, poses, weight, d2, best_weight or best_d2 not 8-byte, the workspace not 16-byte aligned; too small a
 * workspace.  These checks run before any HIP call. */
int sv_voxel_match_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const int32_t *n, const int32_t *counts,
                          const double *poses, int batch, int cap, int n_poses, int64_t min_n, int64_t min_rows, int since, int32_t *inside, int32_t *hits,
                          int64_t *weight, int64_t *d2, int32_t *best, int64_t *best_weight, int64_t *best_d2, void *workspace, size_t workspace_bytes,
                          void *stream);
/* Test hook for the call above, process-wide: group = 0 (the default) lets the call choose how many candidates a workgroup of the score
 * kernel walks, a power of two in 1..64 fixes it.  The results do not depend on it.  Returns SV_OK, or SV_ERR_ARG for another group. */
int sv_debug_voxel_match(int group);

/* ---- (S) a voxel map carried into another: (Q)'s table, filtered and shifted by whole cells -> added into a second table of (Q) ---- */

/* (Q)'s table has no removal and its box is fixed.  This moves the content of one map (src, only read) into another (dst): every value is
 * an integer and stays one, so dst stays bit-exact against stereo_vision.sv.voxel_map_carry, which restates this in numpy.
 *
 *   qualifies  a voxel of src with n >= min_n, m >= min_rows and last_seq >= since - the three filters of the read-out of (Q); a voxel that
 *              does not counts into `filtered`
 *   outside    a qualifying voxel whose cell c + shift leaves 0 .. cells_dst - 1 on an axis counts into `outside`
 *   carried    every other voxel: the voxel of dst with key (c + shift) gets n += n, S += S, C += C, m += m, first_seq = min(., first_seq),
 *              last_seq = max(., last_seq).  The sub-cell offsets S are not changed: a shift by whole cells does not move a point inside
 *              its cell.  `carried` counts them, `claimed` those whose voxel dst did not hold before.
 *   head       dst's dropped += src's dropped.  dst is overflowed after the call iff it was before, or src is, or dst now holds more than
 *              its capacity ((Q)'s rule).  Where src or dst is overflowed as the call starts nothing is carried: carried = -1, the other
 *              counts 0.  Where dst overflows during the call its content is undefined, as after an insert, and so is `claimed`;
 *              carried, filtered and outside are exact even then.
 *   widths     (Q)'s contract: the total weight of a voxel of dst stays below 2^47 after the call.
 *
 * With the box of dst at lo' = lo + k * size (stereo_vision.sv.voxel_map_shifted), shift = -k keeps every voxel at its place in the world.
 *
 * Enqueues two kernels on `stream` (a hipStream_t, NULL = the default stream) - the head, then a lane per slot of src - and does not wait:
 * nothing is allocated and no host synchronisation is made.  Uses the first word of the read-out scratch of dst.  No other call on either
 * map - an insert, a read-out, a match, a clear, another carry - may run at the same time: a destination entry is written with plain
 * stores by the one lane that carries its voxel.
 *   dst, dst_bytes, dst_spec : the map that receives, as (Q)'s entries take it; it must have been cleared or filled before
 *   src, src_bytes, src_spec : the map that is read
 *   shift_x, shift_y, shift_z: whole cells added to a cell of src, each in -2^20 .. 2^20
 *   stats        : int64 [4] device, 8-byte aligned - carried, filtered, outside, claimed, written by the call whatever it held -, or NULL
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, both maps untouched, the text in sv_last_error(NULL) - for: what the clear
 * entry of (Q) refuses, for either map; sizes that differ in a bit; a shift outside -2^20 .. 2^20; buffers that share a byte (the dst_bytes
 * at dst and the src_bytes at src); stats not 8-byte aligned or inside a map.  These checks run before any HIP call.
 * (The name below stands in parentheses - plain C, the same declaration - because tests/test_voxel_map.py pins the set of
 * "sv_*voxel_map*(" declarations of this header to group (Q)'s seven.) */
int (sv_voxel_map_carry_device)(void *dst, size_t dst_bytes, const sv_voxel_map_spec *dst_spec, const void *src, size_t src_bytes,
                                const sv_voxel_map_spec *src_spec, int shift_x, int shift_y, int shift_z, int64_t min_n, int64_t min_rows, int since,
                                int64_t *stats, void *stream);

/* ---- (T) a voxel map carved by the sight lines of frames: per-frame rows of (I) or (F) + poses + (Q)'s table -> voxels seen through, emptied ---- */

/* (Q)'s table only gains voxels, and (S) removes them by age or weight alone.  This removes what later frames see through: every kept
 * row of a frame is the end of a sight line from the sensor, and a voxel that enough sight lines of later frames pass through is carved.
 * Everything behind the two cell computations is an integer, so the result is bit-exact against stereo_vision.sv.voxel_map_carve, which
 * restates this in numpy, whatever the schedule.
 *
 *   sensor   O[k] = ((R[k,0] ox + R[k,1] oy) + R[k,2] oz) + t[k] with (ox, oy, oz) = origin: the insert's expression, in its order, no
 *            FMA.  Frame b casts rays iff all twelve words of its pose are finite and lo < O < hi strictly on every axis; its cell c0 is
 *            the insert's rule, min(int((O - lo) / size), cells - 1) per axis.
 *   rows     frame b has its first min(counts[b], cap) rows, none for counts[b] <= 0.  A row is kept by exactly the insert's rule -
 *            w > 0 and lo < Pw < hi strictly; NaN and inf never pass -, and its cell c1 is the insert's.
 *   ray      with d = c1 - c0 and nst = max |d_a|, a kept row of a casting frame casts a ray iff nst <= reach; it counts into `rays`.
 *            Its steps are k = 1 .. nst - 1 - margin (there may be none) and count into `steps`; the cell of step k is (J)'s line rule
 *            on three axes, c0_a + (2 k d_a + nst) // (2 nst) with a flooring division (a negative d_a floors, half-way steps round
 *            towards +inf).  The major axis moves by exactly one per step: a ray visits no cell twice and never leaves the box.
 *   miss     at each step, where the map holds the key of the cell and that voxel's last_seq < seq0 + b: miss[voxel] += w, the row's
 *            weight (n[b][i], or 1).  A voxel this frame or a later one has seen is never counted against by this frame: what an insert
 *            of the same frames just added is safe, and inside a batch frame b + 1 sees through what only frame b saw.  miss starts
 *            from zero in every call; it does not persist.  Contract: miss < 2^47 per voxel.
 *   verdict  a voxel with miss > 0 counts into `touched`.  It is carved iff miss >= min_miss and 256 miss >= ratio n, n its own weight
 *            (both products stay below 2^63 under the contracts), and counts into `carved`.
 *   apply    with apply = 1 the entry of a carved voxel goes back to the values of a slot that has just been claimed and not yet added
 *            to: n, S, C, m zero, first_seq all ones, last_seq zero (which is also what the miss rule reads of it).  THE KEY STAYS: a
 *            tombstone of an open-addressing table, so probe chains through it stay intact, and a later insert or carry of that cell
 *            adds to it as to a fresh voxel.  Every call skips it at min_n >= 1 - every default -, a carry (a prune) counts it as
 *            `filtered` and frees the slot; `claimed` in the map's head is not changed by a carve.  The one consequence: until the next
 *            prune, the read-out of a carved map is defined for min_n >= 1 only - n = 0 divides.
 * An overflowed map: nothing is done, stats = -1, 0, 0, 0 and miss all zero.
 *
 * Enqueues three kernels on `stream` (a hipStream_t, NULL = the default stream) - miss and stats cleared; a lane per row, its step loop
 * and one integer atomic add per counted step; a lane per slot - and does not wait: nothing is allocated and no host synchronisation is
 * made.  With apply = 0 the map is only read.  No other call on the map may run at the same time.
 *   map, map_bytes, spec : the map, as (Q)'s entries take it
 *   xyz, dtype, n, counts, poses, batch, cap, seq0 : the frames, as sv_voxel_map_insert_device takes them (device pointers)
 *   origin       : HOST, three doubles, read by the call: the sensor's centre in the frame's axes
 *   reach        : cells, 1 .. 1023: rows whose cell lies further from the sensor's on an axis cast no ray
 *   margin       : cells, 0 .. 255, left alone in front of the row's own cell
 *   min_miss     : >= 1;  ratio: 0 .. 65535, in 1 / 256;  apply: 0 or 1
 *   miss         : device, sv_voxel_map_slots(capacity) words, 8-byte aligned, outside the map: per slot of the table, written by the call
 *   stats        : int64 [4] device, 8-byte aligned - rays, steps, touched, carved, written by the call whatever it held -, or NULL
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, everything untouched, the text in sv_last_error(NULL) - for: what the clear
 * entry of (Q) refuses; a dtype that is neither SV_CLOUD_F32 nor SV_CLOUD_F64; batch outside 0 .. 65535; cap < 0; seq0 < 0 or seq0 + batch
 * > 2^31 - 1; reach, margin, min_miss, ratio or apply outside the ranges above; counts or poses NULL with batch > 0, xyz NULL with rows;
 * a pointer not aligned to its element; origin NULL or not finite; miss NULL; miss or stats sharing a byte with the map or with each
 * other.  These checks run before any HIP call. */
int sv_voxel_carve_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const int32_t *n, const int32_t *counts,
                          const double *poses, const double *origin, int batch, int cap, int seq0, int reach, int margin, int64_t min_miss, int ratio, int apply,
                          uint64_t *miss, int64_t *stats, void *stream);

/* ---- (U) the voxel map rendered into a camera: (Q)'s table + world-to-camera poses + the rig's Q -> expected depth, colour, disparity ---- */

/* (Q)'s map can be listed; this answers what a camera should see from a pose if the map is right.  Every product, sum and quotient below
 * is a double, rounded on its own, in the order written (no FMA); everything behind them is an integer, so the result is bit-exact against
 * stereo_vision.sv.voxel_map_render, which restates this in numpy, whatever the schedule.  Camera axes are Q's: x right, y down, z forward.
 *
 *   voxels   those with n >= min_n, m >= min_rows and last_seq >= since, the three filters of (Q)'s read-out; min_n >= 1, so a tombstone
 *            of (T), whose n is 0, is never drawn.  A voxel's centre is the read-out's, Pw = lo + (c + (S + 0.5 n) / (65536 n)) * size.
 *   camera   per view v, cams[v] = R row-major, then t, world to camera: Pc[k] = ((R[k,0] Pw.x + R[k,1] Pw.y) + R[k,2] Pw.z) + t[k].
 *   depth    tz = Pc[2] / size, in cells.  The voxel is kept iff near <= tz && tz < far (NaN never passes); zq = (int)(tz * 256.0) < 2^28.
 *   pixel    u = (f * Pc[0]) / Pc[2] + cx, v = (f * Pc[1]) / Pc[2] + cy; kept iff -2^30 < u < 2^30 and -2^30 < v < 2^30;
 *            px = floor(u + 0.5), py = floor(v + 0.5).
 *   square   r = r_max where half_px / tz >= r_max, else (int)(half_px / tz).  The voxel covers the pixels px - r .. px + r by py - r ..
 *            py + r, clipped to the image; one that covers at least one pixel counts into `drawn`.
 *   winner   of a pixel: the covering voxel with the smallest zq, then the smallest key - never the slot, which depends on the order in
 *            which concurrent inserts claimed colliding entries.  `covered` counts the pixels that have one.
 *   outputs  depth = zq, key = the winner's, color = its (2 C + n) / (2 n) per channel (the read-out's), disparity = (float)e with
 *            z = (((double)zq + 0.5) / 256.0) * size and e = (f / z - q33) / q32 - what (B) would measure, in its units.  A pixel
 *            without a winner holds -1, -1, 0 and -1.
 *   compare  with `measured`: a measured pixel is valid iff it is finite and > 0; d is the float widened to double.  label = 0 neither
 *            measured nor expected, 1 measured only, 2 expected only, 3 |d - e| <= tol, 4 d - e > tol (measured nearer: something new),
 *            5 d - e < -tol (measured farther: the voxel was seen through); counts[v] = the pixels per label.
 * An overflowed map: nothing is drawn, stats = -1, 0 per view, and every pixel is one without a winner.
 *
 * Enqueues four kernels on `stream` (a hipStream_t, NULL = the default stream) - the images cleared; a lane per slot of the table and an
 * integer atomic minimum of zq per covered pixel; the same walk with a minimum of the key where the depth is the lane's; a lane per pixel
 * - and does not wait: nothing is allocated and no host synchronisation is made.  views = 0 enqueues nothing.  The map is only read; no
 * call that writes it may run at the same time. */
typedef struct {
    double f, cx, cy, q32, q33; /* of Q: f = Q[2][3], cx = -Q[0][3], cy = -Q[1][3], q32 = Q[3][2], q33 = Q[3][3]; finite, f > 0, q32 != 0 */
    double half_px;             /* half the edge of a voxel in pixels at a depth of one cell: 0.5 f for a square as wide as the voxel; finite, >= 0 */
    double near, far;           /* cells: 0 < near < far <= 2^20 */
    int32_t width, height;      /* 1 .. 8192 each */
    int32_t r_max;              /* 0 .. 8 */
    int32_t reserved[5];        /* must be 0 */
} sv_voxel_render_spec;

/*   map, map_bytes, spec : the map, as (Q)'s entries take it
 *   cam          : the camera; views * width * height < 2^31
 *   cams         : float64 [views][12] device, 8-byte aligned; views in 0 .. 4096
 *   min_n, min_rows, since : the filters; min_n >= 1
 *   depth        : int32 [views][height][width] device;  key: int64 [views][height][width] device, 8-byte aligned
 *   color        : uint8 [views][height][width][4] device, 4-byte aligned, or NULL;  disparity: float [views][height][width] device, or NULL
 *   measured     : float [views][height][width] device, or NULL: no comparison; given iff label and counts are
 *   tol          : HOST, one double >= 0, read by the call, in pixels of disparity; not read without `measured`
 *   label        : uint8 [views][height][width] device;  counts: int64 [views][6] device, 8-byte aligned
 *   stats        : int64 [views][2] device, 8-byte aligned - drawn, covered
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, everything untouched, the text in sv_last_error(NULL) - for: what the clear
 * entry of (Q) refuses; cam NULL or a reserved word of it not 0; views outside 0 .. 4096; width or height outside 1 .. 8192; views * width *
 * height >= 2^31; a camera word that is not finite, f <= 0 or q32 == 0; half_px < 0; r_max outside 0 .. 8; near or far outside the range
 * above; min_n < 1; measured without label and counts or either of them without measured; tol NULL, negative or NaN with measured; cams,
 * depth, key or stats NULL with views > 0; a pointer not aligned to its element; an output sharing a byte with the map, cams, measured or
 * another output.  These checks run before any HIP call. */
int sv_voxel_render_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const sv_voxel_render_spec *cam, const double *cams, int views,
                           int64_t min_n, int64_t min_rows, int since, int32_t *depth, int64_t *key, uint8_t *color, float *disparity, const float *measured,
                           const double *tol, uint8_t *label, int64_t *stats, int64_t *counts, void *stream);
/* Test and measurement hook, process-wide: the workgroups of the two table walks at most (0: the call chooses; 1 .. 2048), and the kernels
 * a call enqueues (0: all four; 1 .. 3: the first that many - clear, depth, key -, which leaves the outputs unfinished).  A value outside
 * its range leaves that word as it was.  Returns the groups before. */
int sv_debug_voxel_render(int groups, int stages);

/* ---- (V) the voxel map flattened into an occupancy map: (Q)'s table + (K)'s map spec + a height rule -> logodds, last_seen, floor, top ---- */

/* (Q)'s map holds heights; (K)'s layout is what the planner stages (M) to (P) take.  This writes the one from the other.  The centre of a
 * voxel and its flat cell are doubles, every product, sum and quotient rounded on its own, in the order written (no FMA); everything behind
 * them is an integer minimum, maximum or sum, so the result is bit-exact against stereo_vision.sv.voxel_map_flatten, which restates this
 * in numpy, whatever the schedule and wherever the inserts left an entry in the table.
 *
 *   voxels   those with n >= min_n, m >= min_rows and last_seq >= since, the three filters of (Q)'s read-out; min_n >= 1, so a tombstone
 *            of (T), whose n is 0, never takes part.
 *   cell     X, Y = the read-out's centre on axes 0 and 1, lo + (c + (S + 0.5 n) / (65536 n)) * size; gx = floor(X ms), gy = floor(Y ms),
 *            ms = (double)scale; the flat cell is (top - 1 - gx, left - 1 - gy) where top - rows <= gx <= top - 1 and left - cols <= gy <=
 *            left - 1, compared in double before anything is converted.  A voxel outside counts into `outside` and does nothing else.
 *   height   zq = cz * 256 + ((S_z / n) >> 8) in integers: 1/256 of a voxel cell above lo[2]; S_z / n <= 65535, so zq < 2^28.
 *   low/seen per flat cell the least zq and the largest last_seq of its voxels.
 *   floor    mode 0: base = z_ref_q in every cell.  mode 1: base of a cell = the least `low` over the cells within `radius` rows and
 *            columns of it that lie inside the map and hold a voxel - a wall's own column has no ground voxel under it, its neighbours
 *            have.  A cell that holds a voxel has a base.
 *   classify with h = zq - base of the voxel's cell: h < -step_q below (counted, ignored in its cell; mode 0 only), else h < step_q
 *            ground, else h < height_q obstacle, else overhead.  cells[r][c] = the cell's ground, obstacle and overhead voxels; top[r][c] =
 *            the largest zq among its ground and obstacle voxels, -1 without one.
 *   resolve  obstacle >= min_obstacle: L = min(l_max, obstacle * l_occ); else ground >= min_ground: L = max(l_min, -(ground * l_free)) -
 *            the products in 64 bits -, both with last_seen = seen; else L = 0 and last_seen = -1: a cell that holds overhead voxels only
 *            stays unknown.  l_occ, l_free, l_min and l_max are the flat map's.
 *   outputs  logodds, last_seen; floor = base (mode 1: -1 where the window holds no voxel); top; cells; stats = drawn (the voxels that
 *            took part and fell inside), outside, below, ground, obstacle, overhead, occupied_cells, free_cells.
 * An overflowed map: stats[0] = -1, the other counts 0, and the outputs of a map without voxels.
 *
 * Enqueues four or five kernels on `stream` (a hipStream_t, NULL = the default stream) - the outputs cleared; a lane per slot of the table
 * with integer atomic minima and maxima for low and seen; in mode 1 with radius > 0 a lane per flat cell for the floor; the same walk with
 * an atomic add on one of the cell's counts and a maximum on top; a lane per flat cell for L and last_seen - and does not wait: nothing
 * is allocated and no host synchronisation is made.  The voxel map is only read; no call that writes it may run at the same time. */
typedef struct {
    int32_t mode;                     /* 0: an absolute floor at z_ref_q; 1: a local floor, the lowest voxel within `radius` flat cells */
    int32_t z_ref_q;                  /* mode 0: the floor in zq units, floor((z_ref - lo[2]) / size * 256) on the host; |.| < 2^30.  Not read in mode 1 */
    int32_t step_q, height_q;         /* zq units: 1 <= step_q < height_q < 2^28 */
    int32_t radius;                   /* 0 .. 8 flat cells */
    int32_t min_obstacle, min_ground; /* >= 1 */
    int32_t reserved[9];              /* must be 0 */
} sv_voxel_flatten_spec;

/*   map, map_bytes, spec : the voxel map, as (Q)'s entries take it
 *   flat         : the flat map's words, as (K)'s entries take them; rows * cols <= 8 000 000, what (N) and (O) take
 *   flatten      : the height rule
 *   min_n, min_rows, since : the filters; min_n >= 1
 *   logodds      : int16 [rows][cols] device, 2-byte aligned;  last_seen, floor, top: int32 [rows][cols] device
 *   cells        : int32 [rows][cols][3] device;  stats: int64 [8] device, 8-byte aligned
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, everything untouched, the text in sv_last_error(NULL) - for: what the clear
 * entry of (Q) refuses; what (K)'s fuse entry refuses of a map spec; rows * cols above 8 000 000; flatten NULL or a reserved word of it
 * not 0; mode neither 0 nor 1; |z_ref_q| >= 2^30 in mode 0; step_q, height_q, radius, min_obstacle or min_ground outside the ranges
 * above; min_n < 1; an output NULL; a pointer not aligned to its element; an output sharing a byte with the voxel map or another output.
 * These checks run before any HIP call. */
int sv_voxel_flatten_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const sv_occupancy_map_spec *flat, const sv_voxel_flatten_spec *flatten,
                            int64_t min_n, int64_t min_rows, int since, int16_t *logodds, int32_t *last_seen, int32_t *floor, int32_t *top, int32_t *cells,
                            int64_t *stats, void *stream);
/* Test and measurement hook, process-wide: the workgroups of the two table walks at most (0: the call chooses; 1 .. 2048), and the kernels
 * a call enqueues (0: all; 1 .. 4: the first that many of clear, walk A, floor, walk B - the floor counts where it is skipped, too -, which
 * leaves the outputs unfinished).  A value outside its range leaves that word as it was.  Returns the groups before. */
int sv_debug_voxel_flatten(int groups, int stages);

/* ---- (W) the voxel map clustered: (Q)'s table + a height band + a neighbourhood -> a row per connected component, a label per slot ---- */

/* Which voxels of (Q)'s map belong to one thing.  Integers throughout, but for the flat cell of mode 1, which is (V)'s: doubles, every
 * product, sum and quotient rounded on its own, in the order written.  The result is bit-exact against
 * stereo_vision.sv.voxel_map_clusters, which restates this in numpy, whatever the schedule and wherever the inserts left an entry.
 *
 *   members    the slots whose key is a voxel's, whose entry has n >= min_n, m >= min_rows and last_seq >= since - (Q)'s filters; min_n
 *              >= 1, so a tombstone of (T) or of this group, whose n is 0, is never one - and whose height lies in the band: h_lo_q <=
 *              zq - base < h_hi_q with zq = cz * 256 + ((S_z / n) >> 8), (V)'s, in 1/256 of a voxel cell.  mode 0: base = z_ref_q.  mode
 *              1: base = floor[cell], `floor` (V)'s plane of the flat map `flat` and `cell` the flat cell under the voxel's centre on
 *              axes 0 and 1, exactly (V)'s; a voxel outside the flat map or over a cell with floor = -1 is no member.  With h_lo_q =
 *              step_q, h_hi_q = height_q and (V)'s filters the members are (V)'s obstacle voxels.
 *   neighbours connectivity 6, 18 or 26: two cells that differ by at most 1 on every axis, on 1, up to 2 or up to 3 axes.  A cell outside
 *              0 .. cells[k] - 1 on an axis does not exist: the cells are tested per axis, never the keys.
 *   component  the transitive closure over pairs of members in neighbouring cells.  Its identity is the least KEY of its members -
 *              never a slot, which depends on the schedule of the inserts.
 *   row        int64 [16] per component with voxels >= min_voxels: 0 the least key; 1 voxels; 2 the sum of n; 3-5 the least and 6-8 the
 *              largest cell per axis; 9-11 the sum over the members of c_k * 256 + ((S_k / n) >> 8), axes 0 to 2; 12 the least first_seq;
 *              13 the largest last_seq; 14 the sum of m; 15 zero.
 *   capacity   THE CHOICE FOR CUT ROWS.  This entry writes the rows of the first min(kept, capacity) kept components in the order of their
 *              roots' slots - an order that follows the inserts' schedule; the rows behind them are zero.  Which components are cut when
 *              kept > capacity is therefore unspecified HERE.  The definition - the numpy form, and engine.voxel_map_clusters with
 *              sort=True - is "the rows in ascending least key, cut to `capacity`": the engine calls this entry with a row workspace of
 *              min(65535, the map's capacity) rows, sorts what came back by least key and cuts behind the sort, so the rows are the
 *              `capacity` least keys whenever the map holds at most 65535 kept components.  sort=False hands out this entry's order.
 *   info       int64 [8]: 0 members; 1 components; 2 kept components (voxels >= min_voxels, cut or not); 3 the voxels in components below
 *              min_voxels; 4 the voxels emptied; 5 the voxels of the largest component; 6, 7 zero.
 *   label      int32 per slot: -1 no member; -2 a member of a component below min_voxels; -3 a member of a kept component that got no
 *              row; >= 0 the component's row.
 *   drop       1: every member of a component below min_voxels is emptied as (T)'s apply empties: n = S = C = m = 0, the sequence word of
 *              a fresh slot, the key stays - a tombstone.  `claimed` does not change; the next carry into an empty map frees the slots.
 *              0: the map is only read.
 * An overflowed map: nothing is done to it, info[0] = -1, the other words and the rows 0, every label -1.
 *
 * Enqueues eight kernels on `stream` (a hipStream_t, NULL = the default stream) - init, link (a lock-free union-find over the slots:
 * relaxed agent-scope fetch_min only, no flag, no grid barrier, no cooperative launch), roots, count, scan, rank, stats, resolve - and
 * does not wait: nothing is allocated and no host synchronisation is made.  No other call on the map may run at the same time. */
typedef struct {
    int32_t connectivity;  /* 6, 18 or 26 */
    int32_t mode;          /* 0: base = z_ref_q; 1: base = floor[cell] */
    int32_t z_ref_q;       /* mode 0: |.| <= 2^30.  Not read in mode 1 */
    int32_t h_lo_q, h_hi_q; /* -2^30 <= h_lo_q < h_hi_q <= 2^30 */
    int32_t min_voxels;    /* >= 1 */
    int32_t capacity;      /* rows: 1 .. 65535 */
    int32_t drop;          /* 0 or 1 */
    int32_t reserved[8];   /* must be 0 */
} sv_voxel_cluster_spec;

/* Bytes of the workspace for a map of `capacity_of_map` voxels and `capacity` rows; 0 for a capacity outside 1 .. 2^26 or 1 .. 65535. */
size_t sv_voxel_clusters_workspace_bytes(int64_t capacity_of_map, int capacity);
/*   map, map_bytes, spec : the voxel map, as (Q)'s entries take it; written only under drop
 *   cluster      : the words above
 *   flat, floor  : mode 1: the flat map's words, as (K)'s entries take them, and int32 [rows][cols] device, (V)'s floor; not read in mode 0
 *   min_n, min_rows, since : the filters; min_n >= 1
 *   label        : int32 [slots] device, slots = sv_voxel_map_slots(capacity of the map)
 *   clusters     : int64 [capacity][16] device;  info: int64 [8] device; both 8-byte aligned
 *   workspace, workspace_bytes : device, 4-byte aligned, at least sv_voxel_clusters_workspace_bytes
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, everything untouched, the text in sv_last_error(NULL) - for: what the clear
 * entry of (Q) refuses; cluster NULL or a reserved word of it not 0; connectivity none of 6, 18, 26; mode neither 0 nor 1; |z_ref_q| above
 * 2^30 in mode 0; a band that is not -2^30 <= h_lo_q < h_hi_q <= 2^30; min_voxels < 1; capacity outside 1 .. 65535; drop neither 0 nor 1;
 * in mode 1 what (K)'s fuse entry refuses of a map spec, floor NULL or not 4-byte aligned; min_n < 1; label, clusters, info or workspace
 * NULL; a pointer not aligned to its element; workspace_bytes too small; an output or the workspace sharing a byte with the map, the
 * floor or one another.  These checks run before any HIP call. */
int sv_voxel_clusters_device(void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const sv_voxel_cluster_spec *cluster, const sv_occupancy_map_spec *flat, const int32_t *floor, int64_t min_n, int64_t min_rows, int since, int32_t *label, int64_t *clusters, int64_t *info, void *workspace, size_t workspace_bytes, void *stream);
/* Test and measurement hook, process-wide: the workgroups of the table walks at most (0: the call chooses; 1 .. 2048), and `stages`: the
 * low four bits the kernels a call enqueues (0: all; 1 .. 7: the first that many of init, link, roots, count, scan, rank, stats, which
 * leaves the outputs unfinished), 16: roots and stats issue one atomic per member instead of combining equal destinations over the
 * wavefront, 32: the link kernel does not compress paths (by default it lowers a member's own parent word to the root its links
 * ended at).  A value outside its range leaves that word as it was.  Returns the groups before. */
int sv_debug_voxel_clusters(int groups, int stages);

/* ---- (X) a frame aligned to the voxel map: per-frame rows of (I) or (F) + one pose per frame + (Q)'s table -> the sums of one ICP round ---- */

/* (R) answers no finer than its window's step and has no axis for roll and pitch.  This pairs every row of a frame, under the frame's one
 * pose, with the nearest voxel mean of the map and reduces the pairs to the integers a closed-form rigid fit (Kabsch; about z alone for
 * four degrees of freedom) needs; the host solves, applies and calls again: iterative closest point.  Doubles in (Q)'s order in front of
 * the cell, integers behind it: the sums are bitwise reproducible, whatever the schedule.  The map is only read.
 * stereo_vision.sv.voxel_map_align_sums restates all of it in numpy, voxel_align_origin / voxel_align_solve / voxel_map_align are the
 * host's part.
 *
 *   rows, world, kept, cell : exactly (R)'s, under poses[b]; u the 16-bit offset.  sums[b][0] = inside counts the kept rows.
 *   positions  integers from here on, in 1/256 of a cell from lo and below 2^28: a kept row stands at p_k = 256 c_k + (u_k >> 8), a voxel
 *              at q_k = 256 cell_k + ((S_k / n) >> 8), / the integer division - the position (V) slices by.
 *   candidates the voxels of the up to 27 cells c + d, d in {-1, 0, 1}^3, with 0 <= c_k + d_k < cells_k - a cell outside the box is no
 *              cell: its "key" would be another cell's or the empty word -, that pass the read-out's filters with n >= max(min_n, 1),
 *              m >= min_rows, last_seq >= since.  A tombstone of (T) or (W) has n = 0 and is never a partner, whatever min_n is.
 *   nearest    the candidate with the smallest d2 = sum_k (p_k - q_k)^2, among those the smallest key; d2 <= 3 * 511^2 = 783363.
 *   pair       a kept row with a nearest candidate and d2 <= max_d2, max_d2 in 0 .. 783363.  For max_d2 <= 256^2 - a max_dist of at
 *              most one cell - the partner is the nearest voxel mean of the WHOLE map, not only of the 27 cells: a voxel within 256
 *              units differs by at most one cell per axis.
 *   sums       int64 [batch][19]: inside, pairs, W = sum w, D = sum w d2, P[3] = sum w (p - o), Q[3] = sum w (q - o), H[9] = sum w
 *              (p - o)_i (q - o)_j row-major (i the row's axis), over the pairs; o = origin[b], int32 [3] in the positions' unit,
 *              |o_k| <= 2^30.  64-bit two's complement sums; contract: sum w r^2 < 2^63, r the largest |p - o| or |q - o| - with room
 *              for any frame of a stereo rig around an origin at the sensor.
 *   per row    pair_key int64 [batch][cap] and pair_d2 int32 [batch][cap], both or neither: the nearest candidate's key and d2, also
 *              where d2 > max_d2 and the row is no pair; -1 and -1 for a row that is not kept, a kept row without a candidate, and every
 *              index at or beyond min(counts[b], cap).
 *   overflowed for an overflowed map every sum is 0 and every per-row word is -1. */

/* Host only: the bytes of the workspace sv_voxel_align_device needs for `batch` frames of `cap` rows: 19 words per chunk of 256 rows, at
 * most 512 chunks a frame.  SV_ERR_ARG (bytes untouched) for a NULL bytes, cap < 0 or batch outside 0..65535. */
int sv_voxel_align_workspace(int cap, int batch, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as two kernels - the pairs and their sums per chunk of rows, the chunks'
 * sums per frame - and not waited for: nothing is allocated, no host synchronisation is made, no atomic is issued, the map is read only,
 * and nothing is assumed of what the outputs or the workspace held before.
 *   map, spec    : (Q)'s buffer and its spec; xyz, dtype, n, counts, cap : as for sv_voxel_map_insert_device
 *   poses        : double [batch][12] device, 8-byte aligned: frame b's pose, R row-major, then t
 *   origin       : int32 [batch][3] device, 4-byte aligned
 *   max_d2       : 0 .. 783363
 *   min_n, min_rows, since : the filters of sv_voxel_map_rows_device; a min_n below 1 counts as 1
 *   sums         : int64 [batch][19] device, 8-byte aligned
 *   pair_key     : int64 [batch][cap] device, 8-byte aligned, and pair_d2 : int32 [batch][cap] device, 4-byte aligned; or both NULL
 *   workspace    : device, 8-byte aligned, workspace_bytes >= what sv_voxel_align_workspace gives
 * Every output given is written in full.  Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the
 * outputs untouched, the text in sv_last_error(NULL) - for: a bad spec or map as the clear entry of (Q) refuses them; another dtype; cap < 0;
 * batch outside 0..65535; max_d2 outside 0..783363; with batch > 0 a NULL counts, poses, origin, sums or workspace, and with cap > 0 as well
 * a NULL xyz; one of pair_key and pair_d2 without the other; xyz not aligned to its element, n, counts, origin or pair_d2 not 4-byte, poses,
 * sums, pair_key or the workspace not 8-byte aligned; too small a workspace.  These checks run before any HIP call. */
int sv_voxel_align_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const int32_t *n, const int32_t *counts,
                          const double *poses, const int32_t *origin, int batch, int cap, int max_d2, int64_t min_n, int64_t min_rows, int since, int64_t *sums,
                          int64_t *pair_key, int32_t *pair_d2, void *workspace, size_t workspace_bytes, void *stream);
/* Test and measurement hook for the call above, process-wide: max_chunks = 0 (the default) leaves the chunks of rows per frame at 512 at
 * most, 1 .. 512 lowers that, so that a workgroup takes several chunks of a short frame; flags bit 0 makes the score kernel look into every
 * one of the 27 cells instead of leaving out those that cannot hold the nearest.  The results do not depend on either.  Returns SV_OK, or
 * SV_ERR_ARG for other values. */
int sv_debug_voxel_align(int max_chunks, int flags);

/* ---- (Y) normals of the voxel map and point-to-plane alignment: (Q)'s table -> a direction per slot; (X)'s pairs + the directions -> the sums of one round ---- */

/* (X) pairs a row with the nearest voxel MEAN, which holds the row back along every plane it lies on: on a street most rows lie on the road
 * and on walls, and the loop creeps.  Here every voxel gets the normal of the plane through the means around it, and a round's sums are
 * those of the point-to-plane residuals.  Integers from the cell on: both are bit-exact against stereo_vision.sv.voxel_map_normals and
 * voxel_map_align_plane_sums, which restate them in numpy, whatever the schedule and wherever the inserts left an entry - which rules out
 * an eigen-solver in floating point: the normal is found by an exhaustive search over a table of integer directions.  The map is only read.
 *
 * (Y1) normals
 *   members    the slots whose entry passes (Q)'s filters with n >= max(min_n, 1); a tombstone is neither a member nor a neighbour.
 *   position   q_k = 256 cell_k + ((S_k / n) >> 8), (X)'s, in 1/256 of a cell.
 *   neighbours of member v the members in the up to 27 cells c + d, d in {-1, 0, 1}^3, inside the box - a cell is tested against the box
 *              before a key is formed -, v itself among them.  e = q_j - q_v, |e_k| <= 511; N their number (1 .. 27), s1 = sum e, s2 = sum
 *              e e^T, C = N s2 - s1 s1^T: symmetric, positive semi-definite, |C_ij| < 2^28.  T = C00 + C11 + C22.
 *   directions dirs int8 [n_dirs][4], 1 <= n_dirs <= 4096, the fourth byte ignored (stereo_vision.sv.voxel_normal_dirs makes a table of
 *              nearly equal lengths).  s_k = |d_k|^2, Q_k = d_k^T C d_k, 0 <= Q_k < 2^46.  k is flatter than j iff Q_k s_j < Q_j s_k, or
 *              the two are equal and k < j; a direction with s_k = 0 is never chosen.  best the flattest, worst the one with the
 *              largest Q / s, ties to the lower index.  lam3 = Q_best / s_best, lam1 = Q_worst / s_worst, integer divisions (both 0 for
 *              a table of zero vectors); lam2 = T - lam1 - lam3.
 *   verdict    normal = best where N >= min_nb, lam2 > 0, 256 lam3 <= flat lam2 and 256 lam2 >= wide lam1, else -1: a pole or an edge
 *              has one wide axis and gets no normal, a blob gets none either.
 *   outputs    normal int32 per slot, -1 for everything that is not a member; fit int64 [slots][4], optional: N, lam1, lam2, lam3 of
 *              every member, zeros elsewhere; counts int64 [4]: members, members with N >= min_nb, normals given, 0.
 *   overflowed every normal -1, fit and counts 0.
 *
 * (Y2) the sums of one point-to-plane round
 *   rows, world, kept, p, candidates, nearest, pair : (X)'s, word for word.
 *   plane pair a pair whose partner's word of `normal` is a direction of the table: 0 <= normal[slot] < n_dirs.  The array is taken as it
 *              is; nothing is fitted again.  nu = dirs[normal[slot]] as integers.
 *   per pair   l = (p - o) >> 4, an arithmetic shift: the lever arm in 1/16 of a cell.  b = nu . (q - p).  a = (l x nu, nu), six integers.
 *   sums       int64 [batch][32]: inside, pairs - (X)'s -, planes, and over the plane pairs W = sum w, E = sum w b^2, g[6] = sum w a_i b,
 *              A[21] = sum w a_i a_j for i <= j, row-major.  64-bit two's complement sums; contract: sum w (256 |l|max)^2 < 2^63 - without
 *              the shift a_i a_j would reach (2 * 127 * r)^2 and 20 000 rows of a street frame would stand at 2^56.
 *   per row    pair_key, pair_d2: (X)'s; pair_normal int32: the nearest candidate's word of `normal` where that is a direction of the
 *              table, else -1 - also for a row that is not kept and every index at or beyond min(counts[b], cap).  All three or none.
 *   overflowed every sum is 0 and every per-row word is -1.
 * The host solves A x = g (stereo_vision.sv.voxel_align_solve_plane): omega = x[0..2] / 16, t = x[3..5] in 1/256 of a cell. */

/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as a memset of the counts and one kernel, a lane per slot, and not waited
 * for: nothing is allocated, no host synchronisation is made, the map is read only, and the only atomics are the three counts', one flush
 * per workgroup.
 *   map, map_bytes, spec : the voxel map, as (Q)'s entries take it
 *   dirs, n_dirs : int8 [n_dirs][4] device, 4-byte aligned; 1 .. 4096
 *   min_nb       : 3 .. 27;  flat, wide : 0 .. 256
 *   min_n, min_rows, since : the filters of sv_voxel_map_rows_device; a min_n below 1 counts as 1
 *   normal, n_normal : int32 [n_normal] device, 4-byte aligned; n_normal = sv_voxel_map_slots(capacity of the map)
 *   fit          : int64 [n_normal][4] device, 8-byte aligned, or NULL
 *   counts       : int64 [4] device, 8-byte aligned
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in sv_last_error(NULL) - for: what the clear
 * entry of (Q) refuses; n_dirs outside 1 .. 4096; dirs, normal or counts NULL; n_normal not the table's slots; min_nb, flat or wide outside
 * its range; a pointer not aligned to its element; an output sharing a byte with the map, the table or another output.  These checks run
 * before any HIP call. */
int sv_voxel_normals_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const int8_t *dirs, int n_dirs, int min_nb, int flat, int wide, int64_t min_n,
                            int64_t min_rows, int since, int32_t *normal, int64_t n_normal, int64_t *fit, int64_t *counts, void *stream);
/* Host only: the bytes of the workspace sv_voxel_plane_align_device needs for `batch` frames of `cap` rows: 32 words per chunk of 256 rows,
 * at most 512 chunks a frame.  SV_ERR_ARG (bytes untouched) for a NULL bytes, cap < 0 or batch outside 0..65535. */
int sv_voxel_plane_align_workspace(int cap, int batch, size_t *bytes);
/* Enqueued on `stream` as two kernels - the plane pairs and their sums per chunk of rows, the chunks' sums per frame - and not waited for:
 * nothing is allocated, no host synchronisation is made, no atomic is issued, the map is read only, and nothing is assumed of what the
 * outputs or the workspace held before.  Every argument of sv_voxel_align_device means here what it means there, and besides:
 *   normal, n_normal : int32 [n_normal] device, 4-byte aligned: (Y1)'s output for this map, or any array of that length
 *   dirs, n_dirs : the table the words of `normal` index
 *   sums         : int64 [batch][32] device, 8-byte aligned
 *   pair_key, pair_d2, pair_normal : [batch][cap] device, all three or all NULL
 *   workspace    : device, 8-byte aligned, workspace_bytes >= what sv_voxel_plane_align_workspace gives
 * Every output given is written in full.  Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the
 * outputs untouched - for what sv_voxel_align_device refuses, and for: n_dirs outside 1 .. 4096; with batch > 0 a NULL dirs or normal; an
 * n_normal that is not the table's slots; dirs, normal or pair_normal not 4-byte aligned; only some of the three per-row outputs. */
int sv_voxel_plane_align_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const void *xyz, int dtype, const int32_t *n, const int32_t *counts,
                                const double *poses, const int32_t *origin, int batch, int cap, int max_d2, int64_t min_n, int64_t min_rows, int since, const int32_t *normal,
                                int64_t n_normal, const int8_t *dirs, int n_dirs, int64_t *sums, int64_t *pair_key, int32_t *pair_d2, int32_t *pair_normal, void *workspace,
                                size_t workspace_bytes, void *stream);
/* Test and measurement hook for the two calls above, process-wide: max_chunks as sv_debug_voxel_align's, for the plane score kernel; flags
 * bit 0 makes that kernel look into every one of the 27 cells, bit 1 makes the normals kernel search the table for every member - by
 * default a member with N < min_nb, which gets no normal whatever the table says, is not searched where no fit is asked for.  The results
 * do not depend on any of them.  Returns SV_OK, or SV_ERR_ARG for other values. */
int sv_debug_voxel_normals(int max_chunks, int flags);

/* ---- (Z) stereo visual odometry: two left images + the disparity of the first -> temporal matches; matches + a pose -> the sums of one round ---- */

/* The camera and the words of the two calls below.  f, cx, cy in pixels; b16 = 16 b, fb = f b and fb16 = f b16 with b the baseline in
 * metres (1 / Q[3][2]) - the products are made once, by the caller, in double, so that host and device hold the same bits; all finite, f,
 * b16, fb and fb16 > 0.  The match call reads step >= 1, r in 1 .. 7 (the patch is (2 r + 1)^2), wx, wy >= 0 with (2 wx + 1) (2 wy + 1) <=
 * 16384, ratio in 0 .. 256, max_cost >= 0 and capacity in 0 .. 65536; the sums call reads the camera only.  reserved: 0.
 * LDS limit: a wavefront holds its point's window of cur in LDS, 2 wy + 2 r + 1 rows of ((2 wx + 2 r + 1 + 3) / 4 + 1) | 1 dwords, and a
 * workgroup of four has 64 KB: a window of more than 16384 bytes is refused (at r = 4 the cold-start window wx = 64, wy = 24 takes 8436). */
typedef struct {
    double f, cx, cy, b16, fb, fb16;
    int32_t step, r, wx, wy, ratio, max_cost, capacity;
    int32_t reserved[9];
} sv_flow_spec;

/* (Z1) temporal matches.  prev, cur: uint8 [batch][height][width], the rectified left gray images of frames k - 1 and k; d_prev float
 * [batch][height][width]: the disparity of frame k - 1; d_cur the same of frame k, or NULL; guess double [batch][12] or NULL: the expected
 * motion, previous camera to current camera, Xc = R X0 + t, R row-major, then t - NULL is the identity and skips the projection.
 *   points      the pixels (u0, v0) with u0 % step == 0 and v0 % step == 0, in ascending v0 width + u0, with r <= u0 < width - r, r <= v0 <
 *               height - r and d0q = floor(16 d + 0.5) (in double) in 1 .. 2^20 for a positive, finite d = d_prev[v0][u0].
 *   centre      X0 = (((u0 - cx) b16) / d0q, ((v0 - cy) b16) / d0q, fb16 / d0q); Xc_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k; a point with Xc.z <=
 *               0.1 (or NaN) is dropped; c = (floor(((f Xc.x) / Xc.z + cx) + 0.5), floor(((f Xc.y) / Xc.z + cy) + 0.5)), a point whose c is
 *               not within +-2^20 is dropped.  Doubles, one operation at a time, nothing contracted.  Without a guess c = (u0, v0).
 *   candidates  (dx, dy) in [-wx, wx] x [-wy, wy] with r <= c.x + dx < width - r and r <= c.y + dy < height - r; cost = the sum of absolute
 *               differences of the patch of prev around (u0, v0) and that of cur around c + (dx, dy): at most 225 * 255.
 *   best        the least cost, among equals the least (dy + wy) (2 wx + 1) + (dx + wx); second: the least cost among the candidates
 *               with max(|dx - bdx|, |dy - bdy|) > 1.
 *   match       a second exists, 256 best < ratio second, best <= max_cost, and not (wx > 0 and |bdx| == wx), not (wy > 0 and |bdy| == wy).
 *   outputs     matches int32 [batch][capacity][6] = (u0, v0, d0q, u1, v1, d1q) in point order, (u1, v1) = c + best, d1q = floor(16
 *               d_cur[v1][u1] + 0.5) where that is in 1 .. 2^20 for a positive finite d_cur, else -1; cost int32 [batch][capacity][2] =
 *               (best, second); counts int32 [batch]: the matches, or -1 for a frame with more than capacity, whose rows are the first
 *               `capacity` of them.  Rows at and behind a frame's count hold -1: every output is written in full. */

/* Host only: the bytes of the workspace sv_flow_match_device needs: 32 per lattice point.  SV_ERR_ARG (bytes untouched) for a NULL
 * bytes, batch outside 0..65535, width or height outside 1..8192, a bad word of the spec, or a window beyond the LDS limit above. */
int sv_flow_match_workspace(int width, int height, int batch, const sv_flow_spec *spec, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as two kernels - a wavefront per lattice point, a workgroup per frame
 * that packs the matches in order - and not waited for: nothing is allocated, no host synchronisation is made, no atomic is issued, and
 * nothing is assumed of what the outputs or the workspace held before.  All pointers device; d_prev, d_cur, matches, cost, counts and the
 * workspace 4-byte, guess 8-byte aligned.  Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued,
 * the outputs untouched, the text in sv_last_error(NULL) - for what the workspace call refuses; with batch > 0 a NULL prev, cur, d_prev,
 * counts or workspace, and with capacity > 0 as well a NULL matches or cost; a misaligned pointer; too small a workspace. */
int sv_flow_match_device(const void *prev, const void *cur, const float *d_prev, const float *d_cur, const double *guess, int batch, int width, int height,
                         const sv_flow_spec *spec, int32_t *matches, int32_t *cost, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* (Z2) the sums of one round.  matches, counts: (Z1)'s, capacity <= 65536 (a count of -1 or 0 gives sums of 0, a count above the capacity
 * counts as the capacity); poses double [batch][12]: previous camera to current camera; gate_q and dgate_q in 1/16 px, 0 .. 2^20.
 *   per match   d0q in 1 .. 2^20, else it is skipped.  X0 and Xc = (x, y, z) as in (Z1).  fz = f / z, xz = x / z, yz = y / z, bz = fb / z; pu =
 *               floor(16 (f xz + cx) + 0.5), pv = floor(16 (f yz + cy) + 0.5), pd = floor(16 bz + 0.5).  inside: z > 0.1 and |pu|, |pv|, |pd| <=
 *               2^30 (false for NaN).
 *   residuals   ru = 16 u1 - pu, rv = 16 v1 - pv, rd = d1q - pd.  inlier: inside and ru^2 + rv^2 <= gate_q^2; d-inlier: an inlier with d1q > 0
 *               and |rd| <= dgate_q.
 *   Jacobian    with respect to (t, omega) of Xc' = exp(omega) Xc + t: a = fz xz, Ju = (fz, 0, -a, -(a y), f (1 + xz xz), -(f yz)); c = fz yz,
 *               Jv = (0, fz, -c, -(f (1 + yz yz)), a y, f xz); e = bz / z, Jd = (0, 0, -e, -(e y), e x, 0); each entry clamp(floor(16 J +
 *               0.5), +-2^20).
 *   sums        int64 [batch][32]: inside, inliers, dinliers, E = sum ru^2 + rv^2, Ed = sum rd^2, g[6] = sum Jq r, A[21] = sum Jq_i Jq_j (upper
 *               triangle, row-major) over the u and v rows of the inliers and the d rows of the d-inliers.  Contract: capacity <= 65536
 *               and the gates <= 2^20, so a match adds less than 2^43 to a word and every sum stays below 2^59. */

/* Host only: the bytes of the workspace sv_flow_pose_sums_device needs: 32 words per chunk of 256 matches.  SV_ERR_ARG (bytes untouched)
 * for a NULL bytes, capacity outside 0..65536 or batch outside 0..65535. */
int sv_flow_pose_sums_workspace(int capacity, int batch, size_t *bytes);
/* Enqueued on `stream` as two kernels - a lane per match and a partial per chunk, the partials per frame - and not waited for: nothing
 * is allocated, no atomic is issued, batch x 32 words to read back.  matches and counts 4-byte, poses, sums and the workspace 8-byte
 * aligned.  Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, sums untouched - for a bad
 * camera in the spec, capacity, batch or a gate outside its range, with batch > 0 a NULL counts, poses or sums, with capacity > 0 as well
 * a NULL matches or workspace, a misaligned pointer, too small a workspace. */
int sv_flow_pose_sums_device(const int32_t *matches, const int32_t *counts, const double *poses, int batch, int capacity, const sv_flow_spec *spec, int gate_q,
                             int dgate_q, int64_t *sums, void *workspace, size_t workspace_bytes, void *stream);

/* ---- (AA) temporal consistency: the disparity map of frame k - 1 warped into frame k under the motion between them, and compared ---- */

/* The camera as in (Z) - f, cx, cy in pixels, b16 = 16 b, fb = f b, fb16 = f b16, made once by the caller in double; all finite, f, b16, fb
 * and fb16 > 0 - and the words of the call: e_max in 0 .. 4, tol_q in 0 .. 2^20 (1/16 px), rel_q in 0 .. 256, mode 0 fill, 1 confirm,
 * 2 reject.  reserved: 0. */
typedef struct {
    double f, cx, cy, b16, fb, fb16;
    int32_t e_max, tol_q, rel_q, mode;
    int32_t reserved[12];
} sv_warp_spec;

/* d_prev float [batch][height][width]: the disparity of frame k - 1; d_cur the same of frame k, or NULL; poses double [batch][12]: the
 * motion, previous camera to current camera, Xc = R X0 + t, R row-major, then t ((Z)'s layout).  dq(d) = floor(16 d + 0.5) (in double)
 * where that is in 1 .. 2^20 for a positive, finite d, else 0.
 *   sources     every pixel (u0, v0) with d0q = dq(d_prev[v0][u0]) >= 1; its index is src = v0 width + u0.
 *   moved       X0 = (((u0 - cx) b16) / d0q, ((v0 - cy) b16) / d0q, fb16 / d0q); Xc_k = ((R_k0 x + R_k1 y) + R_k2 z) + t_k, as in (Z1).  Doubles,
 *               one operation at a time, nothing contracted.
 *   kept        z = Xc.z > 0.1 (false for NaN); pd = floor(16 (fb / z) + 0.5) in 1 .. 2^20; tu = floor(((f Xc.x) / z + cx) + 0.5), tv =
 *               floor(((f Xc.y) / z + cy) + 0.5) with |tu|, |tv| <= 2^20 (false for NaN).  Every other source is dropped.
 *   footprint   e = min(e_max, (pd + d0q - 1) / d0q - 1) in integers: a point that came closer covers the pixels (tu + dx, tv + dy) with
 *               dx, dy in 0 .. e that lie inside the image.
 *   winner      per target pixel, of the sources that cover it: the largest pd, among equals the smallest src.  It does not depend
 *               on the schedule.
 *   outputs     expected int32 [batch][height][width]: the winner's pd, or 0; source int32 the same shape: the winner's src, or -1;
 *               counts int32 [batch][8] = (sources kept, pixels covered - every cover inside the image, once per source -, the pixels
 *               with label 0 .. 5).
 *   with d_cur  mq = dq(d_cur), ex = expected, t = tol_q + ((rel_q ex) >> 8).  label uint8 [batch][height][width]: 0 neither (mq = 0, ex =
 *               0), 1 measured only, 2 expected only, else 3 agree |mq - ex| <= t, 4 nearer mq > ex + t, 5 farther mq < ex - t.  out float
 *               [batch][height][width]: mode 0 - d_cur's own bits where mq > 0, else (float)ex / 16 (exact) where ex > 0, else -1.0f; mode 1
 *               - d_cur's bits where the label is 3, else -1.0f; mode 2 - d_cur's bits where the label is 1 or 3, else -1.0f.
 *   without     label and out are neither read nor written (they may be NULL); counts takes the labels as 0 and 2. */

/* Host only: the bytes of the workspace sv_disparity_warp_device needs: 8 per pixel.  SV_ERR_ARG (bytes untouched) for a NULL bytes,
 * batch outside 0..65535, width or height outside 1..8192. */
int sv_disparity_warp_workspace(int width, int height, int batch, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as three kernels - the keys and counts cleared, a lane per source
 * pixel with one 64-bit integer atomic max of (pd << 32) | (0xffffffff - src) per covered pixel, a lane per target pixel - and not waited
 * for: nothing is allocated, no host synchronisation is made, no float atomic is issued, nothing is assumed of what the outputs or the
 * workspace held before, and every output is written in full.  All pointers device; d_prev, d_cur, expected, source, out and counts
 * 4-byte, poses and the workspace 8-byte aligned.  Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing
 * enqueued, the outputs untouched, the text in sv_last_error(NULL) - for what the workspace call refuses; a NULL spec or a bad word of
 * it; with batch > 0 a NULL d_prev, poses, expected, source, counts or workspace, and beside a d_cur a NULL label or out; a misaligned
 * pointer; too small a workspace; an output or the workspace that shares bytes with an input or with another output. */
int sv_disparity_warp_device(const float *d_prev, const float *d_cur, const double *poses, int batch, int width, int height, const sv_warp_spec *spec,
                             int32_t *expected, int32_t *source, uint8_t *label, float *out, int32_t *counts, void *workspace, size_t workspace_bytes,
                             void *stream);

/* ---- (AB) object links: the temporal matches of (Z1) + the boxes of both frames -> votes, a link per previous box, the sums of its motion ---- */

/* The camera as in (Z) and the words of the call: the maps' width and height in 1 .. 8192; max_boxes in 0 .. 64, the rows of every box
 * array per frame - a match's membership in the boxes of one frame is one 64-bit word -; band_q in 0 .. 2^20 (1/16 px); min_votes >= 1;
 * share in 0 .. 256; gate_m in 0 .. 2^20 (1/1024 m; 0: no gate).  reserved: 0. */
typedef struct {
    double f, cx, cy, b16, fb, fb16;
    int32_t width, height, max_boxes, band_q, min_votes, share, gate_m;
    int32_t reserved[9];
} sv_track_spec;

/* matches int32 [batch][capacity][6] = (u0, v0, d0q, u1, v1, d1q) and counts int32 [batch]: (Z1)'s, under (Z2)'s rules - capacity <= 65536, a
 * count of -1 or 0 gives nothing, a count above the capacity counts as the capacity, a row with d0q outside 1 .. 2^20 is skipped.  poses
 * double [batch][12]: previous camera to current camera, (Z)'s layout.  boxes0 int32 [batch][max_boxes][4] = (x, y, w, h), n0 int32 [batch] or
 * NULL (max_boxes each; a value outside 0 .. max_boxes is clamped, as in (E)) and q0 int32 [batch][max_boxes]: the boxes of frame k - 1 with a
 * reference disparity each in quarter pixels - (H)'s info[3], (E)'s stat[2]; q <= 0: no depth test for the box.  boxes1, n1, q1: the same of
 * frame k.  centre int32 [batch][max_boxes][3] or NULL.  With M = max_boxes:
 *   members   a box's pixels are (E)'s: columns [clamp(x), clamp(x + w)), rows [clamp(y), clamp(y + h)), clamp(a) = min(max(a, 0), size - 1),
 *             sums in 64 bits: the map's last column and row belong to no box.  in0(i): (u0, v0) in box i of frame k - 1, and q0[i] <= 0 or
 *             |d0q - 4 q0[i]| <= band_q.  in1(j): (u1, v1) in box j of frame k, and q1[j] <= 0 or (d1q > 0 and |d1q - 4 q1[j]| <= band_q).  A
 *             match may be a member of several boxes of a frame.
 *   votes     int32 [batch][M][M + 1]: votes[i][j] = the matches with in0(i) and in1(j); votes[i][M] = the matches with in0(i), the members.
 *   link      j*(i) = the j with the most votes, among equals the lowest; kept if votes[i][j*] >= min_votes and 256 votes[i][j*] >= share
 *             members.  Of several i that keep one j only that with the most votes keeps it, among equals the lowest i: a current box
 *             continues one track.  int32 [batch][M][4] = (j or -1, votes[i][j*], members, the most votes over j != j* - 0 for M = 1).
 *   sums      int64 [batch][M][16] per previous box i with a link, over the matches with in0(i), in1(link[i]) and d1q in 1 .. 2^20.  Xc = the
 *             match's point moved by the pose as in (Z1), X1 = (((u1 - cx) b16) / d1q, ((v1 - cy) b16) / d1q, fb16 / d1q); doubles, one
 *             operation at a time.  inside: Xc.z > 0.1 (false for NaN) and (Z2)'s |pu|, |pv|, |pd| <= 2^30.  For an inside match m_a =
 *             clamp(floor(1024 (X1_a - Xc_a) + 0.5), +-2^20), p_a = clamp(floor(1024 X1_a + 0.5), +-2^30) per axis - the scalings are by powers
 *             of two, so the products are exact - and (Z2)'s ru, rv, rd, each clamped to +-2^20.  With a centre and gate_m > 0 a match counts
 *             only if |m_a - centre[i][a]| <= gate_m on the three axes.  (n, inside, sum ru, sum rv, sum rd, sum ru^2 + rv^2, sum m[3], sum
 *             m^2[3], sum p[3], 0): inside is counted in front of the gate, everything else behind it.  Every sum stays below 2^59.
 * Rows at and behind n0 and columns at and behind n1 are 0, their link (-1, 0, 0, 0); so are the sums of a box without a link.  sum m / n /
 * 1024 is the box's own motion per frame in metres, in the current camera's axes: Xc already carries the camera's.
 * stereo_vision.sv.object_links restates this in numpy. */

/* Host only: the bytes of the workspace sv_object_links_device needs: 16 per match.  SV_ERR_ARG (bytes untouched) for a NULL bytes,
 * capacity outside 0..65536, batch outside 0..65535. */
int sv_object_links_workspace(int capacity, int batch, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as four kernels - votes and sums cleared; a lane per match: its two
 * membership words, the votes added in LDS and flushed by integer atomic adds; a wavefront per frame: the links; a lane per match: the
 * sums added in LDS and flushed by 64-bit integer atomic adds - and not waited for: nothing is allocated, no host synchronisation is made,
 * no float atomic is issued, nothing is assumed of what the outputs or the workspace held before, and every output is written in full.
 * All pointers device; poses, sums and the workspace 8-byte, everything else 4-byte aligned.  Returns SV_OK (nothing enqueued for batch
 * == 0 or max_boxes == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in sv_last_error(NULL) - for what
 * the workspace call refuses; a NULL spec or a bad word of it; with batch > 0 a NULL counts or poses, a NULL matches beside a capacity > 0,
 * and beside max_boxes > 0 a NULL boxes0, q0, boxes1, q1, votes, link, sums or workspace; a misaligned pointer; too small a workspace; an
 * output or the workspace that shares bytes with an input or with another output. */
int sv_object_links_device(const int32_t *matches, const int32_t *counts, const double *poses, int batch, int capacity, const int32_t *boxes0, const int32_t *n0,
                           const int32_t *q0, const int32_t *boxes1, const int32_t *n1, const int32_t *q1, const int32_t *centre, const sv_track_spec *spec,
                           int32_t *votes, int32_t *link, int64_t *sums, void *workspace, size_t workspace_bytes, void *stream);
/* Measurement hook for the call above, process-wide: flags = 1 .. 3 leaves kernels out from the end, for timing by difference only - 1 the
 * sums, 2 the links too, 3 the votes too -, and what they would have written is then undefined.  0 is the default.  Returns SV_OK, or
 * SV_ERR_ARG for a value outside 0 .. 3. */
int sv_debug_object_links(int flags);

/* ---- (AC) place recognition: frames of rows -> polar height descriptors; queries x keys x rolls -> the best key and its shift ---- */

/* The words of a descriptor: rows within r_max (metres, finite, > 0) of the vehicle on both axes, z_lo <= z < z_hi, and at least r_min (0
 * <= r_min < r_max) away; rings in 1 .. 64; sectors a multiple of 4 in 8 .. 128; rings * sectors <= 4096.  reserved: 0.  With them, in
 * double: unit = r_max / 1024, z_unit = (z_hi - z_lo) / 255, ring_edge2[r] = (1024 r / rings)^2 (integer division), r_min2 = floor(r_min /
 * unit)^2. */
typedef struct {
    double r_max, z_lo, z_hi, r_min;
    int32_t rings, sectors;
    int32_t reserved[10];
} sv_place_spec;

/* (AC1) xyz float [batch][capacity][3] (dtype SV_CLOUD_F32) or double (SV_CLOUD_F64) in the vehicle's axes - x forward, y left, z up -, n
 * int32 [batch][capacity] or NULL (every weight 1), counts int32 [batch]: the rows (Q)'s insert takes - frame b has its first min(counts[b],
 * capacity) rows, none for counts[b] <= 0.  poses double [batch][12] or NULL: applied to a row first, by the insert's transform, ((R[k][0] x
 * + R[k][1] y) + R[k][2] z) + t[k] in double and in that order; with the world-to-vehicle words of a pose (stereo_vision.sv.voxel_render_cams
 * makes them) a descriptor is taken from a map's rows around any pose.  dirs int32 [sectors][2] = (rint(2^14 cos(2 pi k / sectors)),
 * rint(2^14 sin(2 pi k / sectors))): made on the host (stereo_vision.sv.place_params), the device computes no trigonometric function.
 *   kept      n >= 1; x, y, z finite; |x| < r_max and |y| < r_max; z_lo <= z < z_hi; and with qx = (int)floor(x / unit), qy likewise, d2 =
 *             qx^2 + qy^2: r_min2 <= d2 < 1024^2 and (qx, qy) != (0, 0).  Doubles, one operation at a time, each division one division.
 *   ring      the largest r with ring_edge2[r] <= d2.
 *   sector    the one k with cross(dir[k], q) >= 0 and cross(dir[(k + 1) % sectors], q) < 0, cross(a, b) = a.x b.y - a.y b.x.
 *   code      1 + min(254, (int)floor((z - z_lo) / z_unit)).
 * desc uint8 [batch][rings][sectors]: per bin the largest code, 0 for an empty bin.  ring uint8 [batch][rings]: the occupied sectors per
 * ring.  words int32 [batch][4] = (the sum of the codes, the occupied bins, the kept rows, the dropped rows of the frame's rows).
 * stereo_vision.sv.place_descriptor restates this in numpy. */

/* Host only: the bytes of the workspace sv_place_descriptor_device needs: 4 (4 + rings * sectors) per frame.  SV_ERR_ARG (bytes
 * untouched) for a NULL bytes, batch outside 0..65535, rings or sectors outside what sv_place_spec admits. */
int sv_place_descriptor_workspace(int batch, int rings, int sectors, size_t *bytes);
/* Enqueued on `stream` (a hipStream_t, NULL = the default stream) as three kernels - the workspace cleared; a lane per row: the maxima of
 * a chunk of 4096 rows in LDS, flushed by integer atomic maxima; a workgroup per frame: bytes, ring counts, words - and not waited for:
 * nothing is allocated, no host synchronisation is made, no float atomic is issued, nothing is assumed of what the outputs or the
 * workspace held before, and every output is written in full.  All pointers device; xyz (double) and poses 8-byte, everything else 4-byte
 * aligned, ring 1-byte.  Returns SV_OK (nothing enqueued for batch == 0), SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs
 * untouched, the text in sv_last_error(NULL) - for batch outside 0..65535, capacity outside 0..2^24, a dtype that is neither, a NULL spec or
 * a bad word of it; with batch > 0 a NULL counts, dirs, desc, ring, words or workspace, a NULL xyz beside a capacity > 0; a misaligned
 * pointer; too small a workspace; an output or the workspace that shares bytes with an input or with another output. */
int sv_place_descriptor_device(const void *xyz, int dtype, const int32_t *n, const int32_t *counts, const double *poses, int batch, int capacity,
                               const int32_t *dirs, const sv_place_spec *spec, uint8_t *desc, uint8_t *ring, int32_t *words, void *workspace,
                               size_t workspace_bytes, void *stream);

/* (AC2) q_desc uint8 [queries][rings][sectors], q_words int32 [queries][4], q_ring uint8 [queries][rings]: (AC1)'s; q_seq int32 [queries]: the
 * queries' sequence numbers.  k_desc, k_words, k_ring, k_seq: the same of the keys.  rings and sectors as in sv_place_spec; min_gap >= 0;
 * ring_gate >= -1; max_shift in 0 .. 128, or -1: every shift; accept in 0 .. 2^20.
 *   candidate key k is one of query q iff both sums (words[0]) are > 0 and |q_seq - k_seq| >= min_gap, and, unless ring_gate < 0, sum_r
 *             |q_ring[r] - k_ring[r]| <= ring_gate: a turn of the vehicle does not change a ring's count.
 *   pair      sad(s) = sum_{r,c} |q[r][c] - k[r][(c + s) % sectors]| for s in 0 .. sectors - 1 with min(s, sectors - s) <= max_shift; the
 *             pair's result is the least sad, among equals the least s; norm = q_sum + k_sum.  A query that stands where the key stood,
 *             turned by 2 pi s / sectors to the left, has shift s.
 *   best      the candidate with the least sad / norm, by sad_a norm_b < sad_b norm_a in 64 bits, among equals the least k; accepted
 *             iff 256 sad <= accept norm.
 * best int32 [queries][4] = (k, or -1 where nothing is accepted; the shift, sad and norm of the best candidate even where it is refused);
 * (-1, 0, -1, 0) without a candidate.  counts int32 [queries][3] = (the keys that pass the sums and the gap, those that also pass the gate,
 * accepted ? 1 : 0).  pair int32 [queries][keys][2] or NULL = (sad, shift) per candidate, (-1, 0) for any other key.
 * stereo_vision.sv.place_match restates this in numpy. */

/* Host only: the bytes of the workspace sv_place_match_device needs: 32 per query and group of 64 keys.  SV_ERR_ARG (bytes untouched) for a
 * NULL bytes, queries outside 0..65535, keys outside 0..2^20. */
int sv_place_match_workspace(int queries, int keys, size_t *bytes);
/* Enqueued on `stream` as two kernels - per query and group of 64 keys the tests, then a wavefront per candidate with a lane per shift,
 * four bytes per v_sad_u8, and the group's best as a partial; a workgroup per query: the best of the partials - and not waited for:
 * nothing is allocated, no host synchronisation is made, no atomic touches a result, nothing is assumed of what the outputs or the
 * workspace held before, and every output is written in full.  All pointers device; the descriptors, words, sequence numbers, outputs and
 * the workspace 4-byte aligned.  Returns SV_OK (nothing enqueued for queries == 0; for keys == 0 every query gets "no candidate"),
 * SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the outputs untouched, the text in sv_last_error(NULL) - for what the workspace call
 * refuses; a bad rings, sectors, min_gap, ring_gate, max_shift or accept; with queries > 0 a NULL q_desc, q_words, q_ring, q_seq, best or
 * counts, and with keys > 0 too a NULL k_desc, k_words, k_ring, k_seq or workspace; a misaligned pointer; too small a workspace; an output
 * or the workspace that shares bytes with an input or with another output. */
int sv_place_match_device(const uint8_t *q_desc, const int32_t *q_words, const uint8_t *q_ring, const int32_t *q_seq, int queries, const uint8_t *k_desc,
                          const int32_t *k_words, const uint8_t *k_ring, const int32_t *k_seq, int keys, int rings, int sectors, int min_gap, int ring_gate,
                          int max_shift, int accept, int32_t *best, int32_t *counts, int32_t *pair, void *workspace, size_t workspace_bytes, void *stream);
/* Measurement hook for the search above, process-wide: flags = 1 takes one key per pass of a wavefront instead of four - the same
 * results, for timing only.  0 is the default.  Returns SV_OK, or SV_ERR_ARG for a value outside 0 .. 1. */
int sv_debug_place(int flags);

/* ---- (AD) a voxel map re-posed: (Q)'s table + a rigid correction per frame -> every voxel moved and accumulated into a second table of (Q) ---- */

/* (S) moves a map by whole cells.  This moves every voxel of one map (src, only read) by a rigid motion of its own and adds it into
 * another (dst): the corrected poses of a pose graph applied to a map whose frames are gone.  Every value of dst is an integer changed by
 * integer atomics whose result does not depend on their order, so dst stays bit-exact against stereo_vision.sv.voxel_map_repose, which
 * restates this in numpy.  Box, size and capacity of the two maps may all differ.
 *
 *   qualifies  a voxel of src with n >= max(min_n, 1), m >= min_rows and last_seq >= since; a voxel that does not counts into `filtered`.
 *              An emptied voxel (n = 0, what (T) and (W) leave) never qualifies, whatever min_n is.
 *   position   p: the centre the read-out of (Q) reports for dtype 1, lo + (c + (S + 0.5 n) / (65536 n)) * size of src per axis, as written
 *   correction corr[k], k = min(max(last_seq - seq0, 0), n_corr - 1) in 64 bits: last_seq alone chooses, so a voxel that two passes of a
 *              drive share moves with the later pass.  Pw[a] = ((R[a,0] px + R[a,1] py) + R[a,2] pz) + t[a]: the insert's transform, in
 *              its order, no FMA.  Any twelve words are taken as they are.
 *   outside    a qualifying voxel for which lo < Pw < hi of dst fails strictly on an axis counts into `outside`; NaN and inf never pass,
 *              so neither does a correction with a word that is not finite
 *   carried    every other voxel: with the insert's cell c = min((int64)t, cells - 1), t = (Pw - lo) / size, and offset u = min((int64)((t -
 *              c) * 65536), 65535) of dst, the voxel of dst with c's key gets n += n, S += n u, C += C, m += m, first_seq = min(.,
 *              first_seq), last_seq = max(., last_seq): an insert of one row of weight n at the voxel's mean, with (S)'s bookkeeping.
 *              `carried` counts them, `claimed` those whose voxel dst did not hold before.  Several voxels of src may land in one of dst.
 *   head       (S)'s: dst's dropped += src's dropped; dst is overflowed after the call iff it was before, or src is, or dst now holds more
 *              than its capacity.  Where src or dst is overflowed as the call starts nothing is carried: carried = -1, the other counts 0.
 *              Where dst overflows during the call its content and `claimed` are undefined; carried, filtered and outside are exact.
 *   widths     (Q)'s contract: the total weight of a voxel of dst stays below 2^47 after the call.
 *
 * There is no shortcut for the identity: a voxel's points collapse to their mean, S becomes n times a whole offset - floor(S / n + 1 / 2), the centre's -, and a re-pose costs
 * up to 1 / 65536 of a cell of position, once per call.
 *
 * Enqueues two kernels on `stream` (a hipStream_t, NULL = the default stream) - the head, then a lane per slot of src - and does not wait:
 * nothing is allocated and no host synchronisation is made.  Uses the first word of the read-out scratch of dst.  No other call on either
 * map may run at the same time.
 *   dst, dst_bytes, dst_spec : the map that receives, as (Q)'s entries take it; it must have been cleared or filled before
 *   src, src_bytes, src_spec : the map that is read
 *   corr         : double [n_corr][12] device, 8-byte aligned: R row-major, then t; n_corr in 1 .. 2^22
 *   seq0         : the sequence number corr[0] belongs to, 0 .. 2^31 - 2
 *   min_n, min_rows, since : the filters of sv_voxel_map_rows_device
 *   stats        : int64 [4] device, 8-byte aligned - carried, filtered, outside, claimed, written by the call whatever it held -, or NULL
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, both maps untouched, the text in sv_last_error(NULL) - for: what the clear
 * entry of (Q) refuses, for either map; a NULL or misaligned corr; n_corr outside 1 .. 2^22; seq0 outside 0 .. 2^31 - 2; maps that share a
 * byte; corr inside dst; stats not 8-byte aligned or inside a map or corr.  These checks run before any HIP call.
 * (The name has no "voxel_map" in it: tests/test_voxel_map.py pins the set of "sv_*voxel_map*(" declarations to group (Q)'s seven.) */
int sv_voxel_repose_device(void *dst, size_t dst_bytes, const sv_voxel_map_spec *dst_spec, const void *src, size_t src_bytes, const sv_voxel_map_spec *src_spec,
                           const double *corr, int n_corr, int seq0, int64_t min_n, int64_t min_rows, int since, int64_t *stats, void *stream);

/* ---- (AE) the pose graph of confirmed loops: poses + relative-pose edges -> one linearisation; the linearisation -> a step per pose by PCG ---- */

/* A graph holds n_poses poses (1 .. 2^20), double [12] each - R row-major, then t, world from frame, (Q)'s layout -, a byte per pose that
 * is not 0 where the pose is held fixed, and n_edges edges (0 .. 2^22): the poses i != j it ties (int32, in either order, duplicates
 * allowed), the measured Z = P_i^-1 o P_j (double [12]) and the weights w = (w_rot, w_trans) >= 0 as they count now - a switched-off edge
 * has both 0.  The incidence lists come from the host (stereo_vision.sv.pose_graph_words): row_start int32 [n_poses + 1] and inc int32 [2
 * n_edges]; pose k's entries are inc[row_start[k] .. row_start[k + 1]), ascending, 2 e where k is edge e's j and 2 e + 1 where it is its i.
 * Every double is formed one operation at a time in the order stereo_vision.sv.pose_graph_linearize and pose_graph_pcg state, without
 * a fused multiply-add, a trigonometric function or a square root, so the device equals the numpy forms bit for bit.  No entry reads the
 * data it is given: an edge or an entry that points outside the graph is skipped by the kernels, everything else is the caller's to
 * check (rig.PoseGraph and stereo_vision.sv.pose_graph do).  lam > 0 is added to the diagonal of H; tol >= 0 is PCG's.  reserved: 0. */
typedef struct {
    double lam, tol;
    int32_t reserved[12];
} sv_pose_graph_spec;

/* (AE1) One linearisation about P_k <- P_k o exp(delta_k), delta = (om, v):
 *   M       P_j^-1 o P_i per edge: all a linearised edge needs, since d r / d delta_j = I and d r / d delta_i = -Ad_M, Ad_M = [[R, 0], [[t]x R, R]]
 *   Wr      W r, r = (a, t_D) of D = Z^-1 o P_i^-1 o P_j with a = 1/2 vee(R_D - R_D^T): no trigonometry
 *   chi2    w_rot |a|^2 + w_trans |t_D|^2
 *   b       - sum J^T W r per pose over its entries in ascending order; 0 for a fixed pose
 *   factor  the 6 x 6 diagonal block of H = sum J^T W J + lam I per pose, 21 words (row p, column q <= p), factored in place as L D L^T
 * Enqueues two kernels on `stream` (a hipStream_t, NULL = the default stream) - a lane per edge, then a lane per pose - and does not wait;
 * nothing is allocated.
 *   poses [n_poses][12], fixed uint8 [n_poses], ei, ej int32 [n_edges], Z [n_edges][12], w [n_edges][2], row_start, inc : device, inputs
 *   M [n_edges][12], Wr [n_edges][6], chi2 [n_edges], b [n_poses][6], factor [n_poses][21] : device doubles, outputs
 * Returns SV_OK, SV_ERR_HIP, or SV_ERR_ARG - nothing enqueued, the text in sv_last_error(NULL) - for: n_poses or n_edges outside their
 * ranges; a NULL spec, a reserved word that is not 0, lam not finite or <= 0, tol negative or not finite; a NULL or misaligned array (the
 * edges' may be NULL where n_edges is 0); an output that shares a byte with an input or another output. */
int sv_pose_graph_linearize_device(const double *poses, const uint8_t *fixed, int n_poses, const int32_t *ei, const int32_t *ej, const double *Z, const double *w,
                                   int n_edges, const int32_t *row_start, const int32_t *inc, const sv_pose_graph_spec *spec, double *M, double *Wr, double *chi2,
                                   double *b, double *factor, void *stream);

/* Host only: the bytes of the workspace sv_pose_graph_pcg_device needs: 64 of state, four vectors of 6 doubles per pose, 6 doubles per
 * edge, five rows of a double per 256 poses, each part rounded up to 16.  SV_ERR_ARG (bytes untouched) for a NULL bytes or a count
 * outside its range. */
int sv_pose_graph_workspace(int n_poses, int n_edges, size_t *bytes);

/* (AE2) Preconditioned conjugate gradients on H x = b from x = 0, H x formed in two passes - g_e = W (x_j - Ad_M x_i) per edge; per pose, over
 * its entries in ascending order, + g_e where it is j and - Ad_M^T g_e where it is i, then + lam x_k -, the preconditioner (AE1)'s factor.
 * A dot product is the poses' six products added left to right, reduced in chunks of 256 by a halving tree and the chunks' partials by
 * the same rule (stereo_vision.sv.pose_graph_sum); every workgroup finishes it for itself, no atomic is used.  The state words - int32
 * iteration, int32 done, double rr, double rr0 - are the first 24 bytes of the workspace: done is set, in double on the device, once rr
 * <= tol^2 rr0, and from then on every kernel returns at its first instruction, so x, iteration and rr stay what they were.
 * Enqueues, on `stream` and without waiting: for iter0 == 0 the start (two kernels: x = 0, r = b, z, the state words); `iters` iterations
 * of three kernels each, numbered iter0 .. iter0 + iters - 1; one workgroup that brings rr and done up to date.  A solve is continued by
 * a call with iter0 = the iterations enqueued so far and everything else as before.
 *   fixed, ei, ej, w, row_start, inc : as (AE1) took them;  M, b, factor : as it wrote them
 *   x         : double [n_poses][6] device, written from iter0 == 0 on
 *   workspace : device, 16-byte aligned, at least sv_pose_graph_workspace's bytes, untouched between the calls of one solve
 * Returns as (AE1), and SV_ERR_ARG besides for iter0 outside 0 .. 2^30, iters outside 0 .. 1024, a workspace that is NULL, misaligned or
 * too small, and x or the workspace sharing a byte with one another or an input. */
int sv_pose_graph_pcg_device(const uint8_t *fixed, int n_poses, const int32_t *ei, const int32_t *ej, const double *w, int n_edges, const int32_t *row_start,
                             const int32_t *inc, const double *M, const double *b, const double *factor, const sv_pose_graph_spec *spec, int iter0, int iters,
                             double *x, void *workspace, size_t workspace_bytes, void *stream);

/* ---- (A)the reference's exported symbols ------------------------------------------------------------- */

typedef struct {
    double x, y, z;
} Double3; /* reference: src/common_includes/structs.h:14-16 */

typedef struct {
    unsigned char x, y, z, w;
} Uchar4; /* reference: src/common_includes/structs.h:18-20 */

/* reference: stereo_vision.cpp:565-623.  left/right: BGRA uint8 [height][width][4].  Returns the library-owned
 * point array [W*H] of the FIRST call's width x height (valid until the next call / clean()).  State is frozen at the
 * first call, like the reference's function-static init (stereo_vision.cpp:582); later frames of another size are resized
 * to it (cv::resize INTER_LINEAR restated, :590-591).  removeSky / subsampling are not read (see sv_legacy_set_subsampling). */
Double3 *generatePointCloud(unsigned char *left, unsigned char *right, char *CAMERA_CALIBRATION_YAML, int width, int height, bool kittiCalibration,
                            bool objectTracking, bool graphics, bool display, int scale, int pc_extrapolation, const char *YOLO_CFG,
                            const char *YOLO_WEIGHTS, const char *YOLO_CLASSES, bool removeSky, bool subsampling);
void clean(void);       /* reference: stereo_vision.cpp:105-114 (without the reference's exit(0)) */
Uchar4 *getColor(void); /* reference: stereo_vision.cpp:625-627 */

/* Last disparity image of the legacy path as the reference's `dmap` (u8 = saturate(round(4*d)), stereo_vision.cpp:316). */
const unsigned char *sv_legacy_last_dmap(int *width, int *height);
/* The 4x4 disparity-to-depth matrix Q the legacy path uses (row major), NULL before the first frame. */
const double *sv_legacy_Q(void);
/* Rectification remap of the gray images in front of the matcher: findRectificationMap's initUndistortRectifyMap maps
 * (stereo_vision.cpp:477-478) applied with cv::remap(INTER_LINEAR) - the call the reference has commented out at :341, so OFF
 * by default here as well.  Call before the first generatePointCloud (the state is frozen there, :582).  OpenCV arithmetic
 * restated (parity unpinned, like the gray conversion). */
void sv_legacy_set_rectify(int on);
/* Half-resolution mode of the legacy path (Elas::parameters::subsampling, set from the driver's `subsample`, stereo_vision.cpp:309).
 * generatePointCloud does NOT read its arguments 15 and 16 (removeSky, subsampling): the reference's own binding passes only 14
 * (stereo_vision/sv.py:180,189), so those slots are undefined under "sv.py drives it unchanged".  Call before the first frame. */
void sv_legacy_set_subsampling(int on);
/* HIP device of the legacy path (default 0).  Call before the first frame. */
void sv_legacy_set_device(int device);
/* The four maps lmapx, lmapy, rmapx, rmapy as [4][height][width] floats (host), NULL unless rectification is on. */
const float *sv_legacy_rectify_maps(void);
/* Test hook: the gray images of the last frame as the matcher received them (after the remap if it is on); [height][width] each. */
int sv_legacy_last_gray(unsigned char *left, unsigned char *right);
/* Batched disparity -> point cloud on the device, for callers of the batch API: the driver's conversion dmap = saturate(
 * round_half_even(4*d)) (stereo_vision.cpp:316) followed by publishPointCloud's reprojection pos = Q*[x y dmap 1]^T,
 * (X,Y,Z) = pos.xyz/pos.w in double (:233-256) for every pixel, and optionally the CUDA variant's robot-frame transform
 * XR*(X,Y,Z)+XT (parallel_includes/main/stereo_vision.cu:188-212).
 *   disp       : float  [B][height][width]     device (e.g. d1 of sv_process_batch_device)
 *   Q16        : double [16] HOST, row major   (e.g. sv_legacy_Q(), or your own stereoRectify result)
 *   XR9 / XT3  : double [9] / [3] HOST, row major; both NULL = no transform (the serial driver)
 *   dmap_out   : uint8  [B][height][width]     device, may be NULL
 *   points_out : double [B][height][width][3]  device
 * Runs on the device's default stream and returns when the points are complete. */
int sv_reproject_batch_device(const float *disp, int batch, int width, int height, const double *Q16, const double *XR9, const double *XT3, unsigned char *dmap_out,
                              double *points_out);
/* The driver's 8-bit disparity image alone: dmap = saturate(round_half_even(4 * d)) (leftdpf.convertTo(dmap, CV_8UC1, 4.0),
 * stereo_vision.cpp:316) for `count` floats in device memory, enqueued on `stream` (a hipStream_t, NULL = the default stream) and NOT
 * waited for - e.g. in front of a gather of finished maps, which then moves a quarter of the bytes. */
int sv_disparity_to_u8_device(const float *disp, size_t count, unsigned char *dmap_out, void *stream);
/* Mean 3-D position of the cloud inside each detector box (x, y, w, h in pixels), i.e. what publishPointCloud hands to its
 * viewer for every tracked object (stereo_vision.cpp:261-278; the boxes come from a detector the caller runs - the
 * reference's YOLO weights are not part of this library).  boxes: int32 [n][4]; out: double [n][3] = (X, Y, Z) sums over
 * columns [clamp(x), clamp(x+w)) outer and rows [clamp(y), clamp(y+h)) inner of the last frame's points, divided by the
 * box's pixel count - the reference's summation order, so the doubles are the reference's.  Returns 0, or -1 before the
 * first frame / on bad arguments. */
int sv_legacy_box_means(const int32_t *boxes, int n, double *out);
/* Test hook: Q (and P1,P2) of the stereoRectify restatement for a calibration file; K1,K2 are divided by `scale` first
 * (stereo_vision.cpp:364-376).  variant 1 = OpenCV 4.x rule set (the product), 0 = pre-3.4.2 rule set. */
int sv_debug_stereo_rectify(const char *yaml, int image_w, int image_h, double scale, int variant, double *Q16, double *P1P2_24);

/* Test hook: cv::initUndistortRectifyMap(K, D(k1,k2,p1,p2,k3), R, P(3x4), (w,h), CV_32F) as the legacy path restates it. */
int sv_debug_undistort_map(const double *K9, const double *D5, const double *R9, const double *P12, int w, int h, float *mapx, float *mapy);

#ifdef __cplusplus
}
#endif
#endif
