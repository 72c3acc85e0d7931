// Group (P) of include/stereo_vision_hip.h: the expected view of the world map from candidate poses (view_kernels.hip).  Everything here
// is argument checking and launch set-up; every check runs before anything is enqueued, a refused call leaves its text for
// sv_last_error(NULL), and no entry waits for the GPU.
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "view_kernels.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_variant{sv::VIEW_WINDOW_BY_REACH};
std::atomic<int> g_stages{3};

// The workspace: a byte per cell for the states, then a score per candidate - for as many as a call may have, so that the size depends
// on the map alone.
size_t state_bytes(int rows, int cols) { return align16((size_t)rows * cols); }
size_t score_bytes() { return align16((size_t)sv::VIEW_POSES_MAX * sizeof(int32_t)); }

}  // namespace

extern "C" {

int sv_view_workspace(int rows, int cols, size_t *bytes) {
    if (!bytes) return refuse("sv_view_workspace: bytes is NULL");
    if (const char *bad = check_map_shape("sv_view_workspace", rows, cols)) return refuse(bad);
    *bytes = state_bytes(rows, cols) + score_bytes();
    return SV_OK;
}

int sv_view_device(const int16_t *logodds, const int32_t *last_seen, const sv_occupancy_map_spec *map, const double *poses, int n_groups, int n_poses,
                   const double *ends, int n_rays, int reach, int occupied, int free_, int max_unknown, int32_t *counts, int16_t *end_cells, uint8_t *status,
                   int32_t *best, int32_t *best_score, void *workspace, size_t workspace_bytes, void *stream) {
    if (const char *bad = check_map("sv_view", map)) return refuse(bad);
    if (n_poses < 1) return refuse("sv_view: n_poses < 1");
    if (n_groups < 0 || (int64_t)n_groups * n_poses > sv::VIEW_POSES_MAX) return refuse("sv_view: n_groups * n_poses outside 0..65535");
    if (n_rays < 1 || n_rays > sv::VIEW_RAYS_MAX) return refuse("sv_view: n_rays outside 1..1024");
    if (reach < 1 || reach > sv::VIEW_REACH_MAX) return refuse("sv_view: reach outside 1..254");
    if (max_unknown < 0 || max_unknown > 255) return refuse("sv_view: max_unknown outside 0..255");
    if (!logodds || !last_seen || !ends || !workspace) return refuse("sv_view: logodds, last_seen, ends or the workspace is NULL");
    if (n_groups > 0 && (!poses || !counts || !end_cells || !status || !best || !best_score))
        return refuse("sv_view: poses, counts, end_cells, status, best or best_score is NULL");
    if (misaligned(logodds, 2)) return refuse("sv_view: logodds is not 2-byte aligned");
    if (misaligned(last_seen, 4)) return refuse("sv_view: last_seen is not 4-byte aligned");
    if (any_misaligned(8, poses, ends)) return refuse("sv_view: poses or ends is not 8-byte aligned");
    if (any_misaligned(4, counts, end_cells, best, best_score))
        return refuse("sv_view: counts, end_cells, best or best_score is not 4-byte aligned");
    if (misaligned(workspace, 16)) return refuse("sv_view: the workspace is not 16-byte aligned");
    const size_t states = state_bytes(map->rows, map->cols), need = states + score_bytes();
    if (workspace_bytes < need) return refuse("sv_view: the workspace is smaller than sv_view_workspace asks for");
    const size_t cells = (size_t)map->rows * map->cols, K = (size_t)n_groups * n_poses;
    const Span spans[10] = {{logodds, cells * 2}, {last_seen, cells * 4}, {poses, K * 32}, {ends, (size_t)n_rays * 16}, {counts, K * 12}, {end_cells, K * n_rays * 4},
                            {status, K * n_rays}, {best, (size_t)n_groups * 4}, {best_score, (size_t)n_groups * 4}, {workspace, need}};
    if (outputs_overlap(spans, 10, 4))  // counts is the first output
        return refuse("sv_view: counts, end_cells, status, best, best_score and the workspace overlap one another or an input");
    if (n_groups == 0) return SV_OK;  // nothing to do

    sv::ViewArgs a;
    memset(&a, 0, sizeof(a));
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    a.logodds = logodds, a.last_seen = last_seen, a.state = ws, a.score = reinterpret_cast<int32_t *>(ws + states);
    a.poses = poses, a.ends = ends, a.counts = counts, a.end_cells = end_cells, a.status = status, a.best = best, a.best_score = best_score;
    a.m = sv::map_cells_of(*map);
    a.G = n_groups, a.P = n_poses, a.n_rays = n_rays, a.reach = reach, a.occupied = occupied, a.free_ = free_, a.max_unknown = max_unknown;
    a.window = g_variant.load() == sv::VIEW_WINDOW_FULL ? (int)sv::VIEW_REACH_MAX : reach;
    if (sv::launch_view(a, static_cast<hipStream_t>(stream), g_stages.load()) != hipSuccess) {
        sv_internal_set_error("sv_view: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_view(int variant, int stages) {
    if (variant != sv::VIEW_WINDOW_BY_REACH && variant != sv::VIEW_WINDOW_FULL)
        return refuse("sv_debug_view: variant must be 0 (the window sized by reach) or 1 (always 509 cells a side)");
    if (stages < 1 || stages > 3) return refuse("sv_debug_view: stages must be 1 (the state plane), 2 (and the walk) or 3 (and the best: the whole call)");
    g_variant.store(variant);
    g_stages.store(stages);
    return SV_OK;
}

} /* extern "C" */
