// Group (V) of include/stereo_vision_hip.h: a voxel map of (Q) flattened into an occupancy map of (K) (voxel_flatten_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).  The checks of the voxel map's spec and buffer and of the flat map's spec are stage_glue.h's.
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_flatten_kernels.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_groups{0};  // sv_debug_voxel_flatten: the workgroups of a table walk at most, 0 = VFLATTEN_MAX_GROUPS
std::atomic<int> g_stages{0};  // and the kernels a call enqueues, 0 = all

}  // namespace

extern "C" {

int sv_voxel_flatten_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const sv_occupancy_map_spec *flat, const sv_voxel_flatten_spec *flatten,
                            int64_t min_n, int64_t min_rows, int since, int16_t *logodds, int32_t *last_seen, int32_t *floor, int32_t *top, int32_t *cells,
                            int64_t *stats, void *stream) {
    int nc[3], l;
    if (const char *bad = check_voxel_map("sv_voxel_flatten", map, map_bytes, spec, nc, &l)) return refuse(bad);
    if (const char *bad = check_map("sv_voxel_flatten", flat)) return refuse(bad);
    if ((int64_t)flat->rows * flat->cols > sv::VFLATTEN_CELLS_MAX) return refuse("sv_voxel_flatten: rows * cols of the map above 8 000 000");
    if (!flatten) return refuse("sv_voxel_flatten: flatten is NULL");
    for (int k = 0; k < 9; k++)
        if (flatten->reserved[k] != 0) return refuse("sv_voxel_flatten: a reserved word of flatten is not 0");
    if (flatten->mode != 0 && flatten->mode != 1) return refuse("sv_voxel_flatten: mode is neither 0 nor 1");
    if (flatten->mode == 0 && (flatten->z_ref_q <= -(1 << 30) || flatten->z_ref_q >= (1 << 30))) return refuse("sv_voxel_flatten: |z_ref_q| is 2^30 or more");
    if (!(1 <= flatten->step_q && flatten->step_q < flatten->height_q && flatten->height_q < (1 << 28)))
        return refuse("sv_voxel_flatten: step_q and height_q need 1 <= step_q < height_q < 2^28");
    if (flatten->radius < 0 || flatten->radius > sv::VFLATTEN_RADIUS_MAX) return refuse("sv_voxel_flatten: radius outside 0..8");
    if (flatten->min_obstacle < 1 || flatten->min_ground < 1) return refuse("sv_voxel_flatten: min_obstacle or min_ground < 1");
    if (min_n < 1) return refuse("sv_voxel_flatten: min_n < 1");
    if (!logodds || !last_seen || !floor || !top || !cells || !stats) return refuse("sv_voxel_flatten: logodds, last_seen, floor, top, cells or stats is NULL");
    if (misaligned(stats, 8)) return refuse("sv_voxel_flatten: stats is not 8-byte aligned");
    if (any_misaligned(4, last_seen, floor, top, cells)) return refuse("sv_voxel_flatten: last_seen, floor, top or cells is not 4-byte aligned");
    if (misaligned(logodds, 2)) return refuse("sv_voxel_flatten: logodds is not 2-byte aligned");
    const size_t n_cells = (size_t)flat->rows * flat->cols;
    const Span spans[] = {{map, map_bytes}, {logodds, n_cells * 2}, {last_seen, n_cells * 4}, {floor, n_cells * 4}, {top, n_cells * 4}, {cells, n_cells * 12},
                          {stats, sv::VFLATTEN_STATS * sizeof(int64_t)}};
    if (outputs_overlap(spans, 7, 1)) return refuse("sv_voxel_flatten: an output shares a byte with the map or another output");

    sv::VoxelFlattenArgs a;
    memset(&a, 0, sizeof(a));
    a.map = static_cast<const uint8_t *>(map);
    a.log2_slots = l, a.size = spec->size;
    for (int k = 0; k < 3; k++) a.lo[k] = spec->lo[k];
    a.min_n = min_n, a.min_rows = min_rows, a.since = since;
    a.m = sv::map_cells_of(*flat);
    a.l_occ = flat->l_occ, a.l_free = flat->l_free, a.l_min = flat->l_min, a.l_max = flat->l_max;
    a.mode = flatten->mode, a.z_ref_q = flatten->mode == 0 ? flatten->z_ref_q : 0, a.step_q = flatten->step_q, a.height_q = flatten->height_q, a.radius = flatten->radius;
    a.min_obstacle = flatten->min_obstacle, a.min_ground = flatten->min_ground;
    a.logodds = logodds, a.last_seen = last_seen, a.floor = floor, a.top = top, a.cells = cells;
    a.stats = reinterpret_cast<long long *>(stats);
    const int groups = g_groups.load();
    if (sv::launch_voxel_flatten(a, groups ? groups : sv::VFLATTEN_MAX_GROUPS, g_stages.load(), static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_flatten: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_voxel_flatten(int groups, int stages) {
    if (stages >= 0 && stages < sv::VFLATTEN_STAGES) g_stages.store(stages);
    if (groups < 0 || groups > sv::VFLATTEN_MAX_GROUPS) return g_groups.load();
    return g_groups.exchange(groups);
}

} /* extern "C" */
