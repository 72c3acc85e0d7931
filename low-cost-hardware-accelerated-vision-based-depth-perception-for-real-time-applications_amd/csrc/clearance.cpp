// Group (M) of include/stereo_vision_hip.h: the obstacle-clearance field of the world map and the footprint check of candidate paths
// (clearance_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a
// refused call leaves its text for sv_last_error(NULL).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "clearance_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_variant{sv::CLEARANCE_AUTO};
std::atomic<unsigned long long *> g_taps{nullptr};

}  // namespace

extern "C" {

int sv_clearance_workspace(int rows, int cols, size_t *bytes) {
    if (!bytes) return refuse("sv_clearance_workspace: bytes is NULL");
    if (const char *bad = check_map_shape("sv_clearance_workspace", rows, cols)) return refuse(bad);
    *bytes = align16((size_t)rows * cols);  // the column pass's byte per cell
    return SV_OK;
}

int sv_clearance_device(const int16_t *logodds, const int32_t *last_seen, int rows, int cols, int radius, int t_occ, int unknown, uint16_t *d2, void *workspace,
                        size_t workspace_bytes, void *stream) {
    if (!logodds || !d2 || !workspace) return refuse("sv_clearance: logodds, d2 or the workspace is NULL");
    if (const char *bad = check_map_shape("sv_clearance", rows, cols)) return refuse(bad);
    if (radius < 1 || radius > sv::CLEARANCE_MAX_R) return refuse("sv_clearance: radius outside 1..254");
    if (t_occ < -32768 || t_occ > 32767) return refuse("sv_clearance: t_occ outside the int16 range");
    if (unknown != 0 && unknown != 1) return refuse("sv_clearance: unknown is neither 0 nor 1");
    if (unknown == 1 && !last_seen) return refuse("sv_clearance: unknown == 1 needs last_seen");
    if (misaligned(logodds, 2)) return refuse("sv_clearance: logodds is not 2-byte aligned");
    if (misaligned(last_seen, 4)) return refuse("sv_clearance: last_seen is not 4-byte aligned");
    if (misaligned(d2, 2)) return refuse("sv_clearance: d2 is not 2-byte aligned");
    if (misaligned(workspace, 16)) return refuse("sv_clearance: the workspace is not 16-byte aligned");
    const size_t cells = (size_t)rows * cols, need = align16(cells);
    if (workspace_bytes < need) return refuse("sv_clearance: the workspace is smaller than sv_clearance_workspace asks for");
    if (overlap(d2, cells * 2, logodds, cells * 2) || overlap(d2, cells * 2, last_seen, cells * 4) || overlap(d2, cells * 2, workspace, need))
        return refuse("sv_clearance: d2 overlaps logodds, last_seen or the workspace");

    sv::ClearanceArgs a;
    memset(&a, 0, sizeof(a));
    a.logodds = logodds, a.last_seen = last_seen, a.g = static_cast<uint8_t *>(workspace), a.d2 = d2;
    a.taps = g_taps.load();
    a.rows = rows, a.cols = cols, a.R = radius, a.t_occ = t_occ, a.unknown = unknown;
    const int variant = g_variant.load();
    a.early_exit = variant != sv::CLEARANCE_TWO_PASS_FULL;
    // the call's own choice is the two kernels at every radius (DESIGN.md §4l has the measurement); the fused kernel where the test hook
    // asks for it and its halo fits
    const bool fused = variant == sv::CLEARANCE_FUSED && radius <= sv::CLEARANCE_FUSED_MAX_R;
    int passes = 3;
    if (const char *s = getenv("SV_CLEARANCE_PASS")) passes = !strcmp(s, "cols") ? 1 : !strcmp(s, "rows") ? 2 : 3;
    if (sv::launch_clearance(a, static_cast<hipStream_t>(stream), fused, passes) != hipSuccess) {
        sv_internal_set_error("sv_clearance: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_clearance_paths_device(const uint16_t *d2, const sv_occupancy_map_spec *map, const double *poses, int n_paths, int n_steps, const double *centres,
                              const int32_t *r2, int n_discs, int radius, int32_t *first_hit, int32_t *min_d2, int32_t *n_outside, void *stream) {
    if (const char *bad = check_map("sv_clearance_paths", map)) return refuse(bad);
    if (n_paths < 0 || n_paths > 65535) return refuse("sv_clearance_paths: n_paths outside 0..65535");
    if (n_steps < 1 || n_steps > 65535) return refuse("sv_clearance_paths: n_steps outside 1..65535");
    if (n_discs < 1 || n_discs > sv::CLEARANCE_MAX_DISCS) return refuse("sv_clearance_paths: n_discs outside 1..64");
    if (radius < 1 || radius > sv::CLEARANCE_MAX_R) return refuse("sv_clearance_paths: radius outside 1..254");
    if (!d2 || !centres || !r2) return refuse("sv_clearance_paths: d2, centres or r2 is NULL");
    if (n_paths > 0 && (!poses || !first_hit || !min_d2 || !n_outside)) return refuse("sv_clearance_paths: poses, first_hit, min_d2 or n_outside is NULL");
    if (misaligned(d2, 2)) return refuse("sv_clearance_paths: d2 is not 2-byte aligned");
    if (any_misaligned(8, poses, centres)) return refuse("sv_clearance_paths: poses or centres is not 8-byte aligned");
    if (any_misaligned(4, r2, first_hit, min_d2, n_outside))
        return refuse("sv_clearance_paths: r2, first_hit, min_d2 or n_outside is not 4-byte aligned");
    for (int k = 0; k < n_discs; k++)
        if (r2[k] < 0 || r2[k] > radius * radius) return refuse("sv_clearance_paths: an r2 is negative or above radius^2, where a saturated cell would hide a hit");
    if (n_paths == 0) return SV_OK;  // nothing to do

    sv::ClearancePathsArgs a;
    memset(&a, 0, sizeof(a));
    a.d2 = d2, a.poses = poses, a.first_hit = first_hit, a.min_d2 = min_d2, a.n_outside = n_outside;
    a.n_paths = n_paths, a.n_steps = n_steps, a.n_discs = n_discs;
    a.m = sv::map_cells_of(*map);
    sv::ClearanceDiscs discs;
    memset(&discs, 0, sizeof(discs));
    for (int k = 0; k < n_discs; k++) discs.px[k] = centres[2 * k], discs.py[k] = centres[2 * k + 1], discs.r2[k] = r2[k];
    if (sv::launch_clearance_paths(a, discs, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_clearance_paths: a launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_clearance(int variant, unsigned long long *taps_device) {
    if (variant < sv::CLEARANCE_AUTO || variant > sv::CLEARANCE_TWO_PASS_FULL) return refuse("sv_debug_clearance: variant must be 0 (the call chooses), 1, 2 or 3");
    g_variant.store(variant);
    g_taps.store(taps_device);
    return SV_OK;
}

} /* extern "C" */
