// Group (K) of include/stereo_vision_hip.h: per-frame occupancy grids fused into a world-fixed log-odds map (occupancy_map_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "occupancy_map_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_cull{1};
std::atomic<unsigned long long *> g_lookups{nullptr};

static_assert(MAP_CELL_MAX == sv::OCCMAP_CELL_MAX, "check_map admits the offsets the kernel can address");

}  // namespace

extern "C" {

int sv_occupancy_fuse_device(const uint8_t *state, const double *poses, int batch, int seq0, const sv_occupancy_spec *frame, const sv_occupancy_map_spec *map,
                              int shift_rows, int shift_cols, const int16_t *logodds_in, const int32_t *last_seen_in, int16_t *logodds_out,
                              int32_t *last_seen_out, void *stream) {
    int frows, fcols;
    if (!frame) return refuse("sv_occupancy_fuse: the frame spec is NULL");
    if (sv_occupancy_dims(frame, &frows, &fcols) != SV_OK) return refuse("sv_occupancy_fuse: the frame spec is not one sv_occupancy_dims admits");
    if (const char *bad = check_map("sv_occupancy_fuse", map)) return refuse(bad);
    if (batch < 0 || batch > 65535) return refuse("sv_occupancy_fuse: batch outside 0..65535");
    if (seq0 < 0 || seq0 > INT_MAX - batch) return refuse("sv_occupancy_fuse: seq0 < 0 or seq0 + batch overflows");
    if (batch > 0 && (!state || !poses)) return refuse("sv_occupancy_fuse: state or poses is NULL");
    if (!logodds_in || !logodds_out) return refuse("sv_occupancy_fuse: logodds_in or logodds_out is NULL");
    if ((last_seen_in == nullptr) != (last_seen_out == nullptr)) return refuse("sv_occupancy_fuse: only one of last_seen_in and last_seen_out is given");
    if (misaligned(poses, 8)) return refuse("sv_occupancy_fuse: poses is not 8-byte aligned");
    if (any_misaligned(2, logodds_in, logodds_out)) return refuse("sv_occupancy_fuse: logodds_in or logodds_out is not 2-byte aligned");
    if (any_misaligned(4, last_seen_in, last_seen_out))
        return refuse("sv_occupancy_fuse: last_seen_in or last_seen_out is not 4-byte aligned");
    const size_t cells = (size_t)map->rows * map->cols;
    const bool shifted = shift_rows != 0 || shift_cols != 0;
    // in place is one lane reading and writing its own cell: only with a zero shift and the very same buffers
    if (overlap(logodds_in, cells * 2, logodds_out, cells * 2) && (shifted || logodds_in != logodds_out))
        return refuse("sv_occupancy_fuse: logodds_in and logodds_out overlap (allowed only as the same buffer with a zero shift)");
    if (last_seen_in && overlap(last_seen_in, cells * 4, last_seen_out, cells * 4) && (shifted || last_seen_in != last_seen_out))
        return refuse("sv_occupancy_fuse: last_seen_in and last_seen_out overlap (allowed only as the same buffer with a zero shift)");
    if (batch == 0 && !shifted && logodds_in == logodds_out && last_seen_in == last_seen_out) return SV_OK;  // nothing to do

    sv::OccupancyMapArgs a;
    memset(&a, 0, sizeof(a));
    a.state = state, a.poses = poses;
    a.logodds_in = logodds_in, a.last_seen_in = last_seen_in, a.logodds_out = logodds_out, a.last_seen_out = last_seen_out;
    a.lookups = g_lookups.load();
    a.B = batch, a.seq0 = seq0;
    a.rows = map->rows, a.cols = map->cols, a.top = map->top, a.left = map->left;
    a.shift_rows = shift_rows, a.shift_cols = shift_cols;
    a.frows = frows, a.fcols = fcols;
    a.l_occ = map->l_occ, a.l_free = map->l_free, a.l_min = map->l_min, a.l_max = map->l_max;
    a.half = 1.0 / (2.0 * (double)map->scale);
    a.fx0 = frame->x_range[0], a.fx1 = frame->x_range[1], a.fy0 = frame->y_range[0], a.fy1 = frame->y_range[1];
    a.fs = (double)frame->scale;
    a.fr1 = trunc(a.fx1 * a.fs), a.fc1 = trunc(a.fy1 * a.fs);  // |.| <= 2^46: exact
    a.cell = 2.0 * a.half;
    // the strip's own extent instead of that of its centres: a little more than needed
    a.reach = 0.5 * sqrt((double)(sv::OCCMAP_WAVE_ROWS * sv::OCCMAP_WAVE_ROWS + sv::OCCMAP_TILE_COLS * sv::OCCMAP_TILE_COLS)) * a.cell;

    if (sv::launch_occupancy_fuse(a, g_cull.load() != 0, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_occupancy_fuse: the kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_occupancy_fuse(int cull, unsigned long long *lookups_device) {
    g_cull.store(cull != 0 ? 1 : 0);
    g_lookups.store(lookups_device);
    return SV_OK;
}

} /* extern "C" */
