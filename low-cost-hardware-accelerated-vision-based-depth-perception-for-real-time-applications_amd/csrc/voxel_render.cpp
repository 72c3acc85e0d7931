// Group (U) of include/stereo_vision_hip.h: a voxel map of (Q) rendered into a camera (voxel_render_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).  The check of a map's spec and buffer is stage_glue.h's.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "voxel_render_kernels.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_groups{0};  // sv_debug_voxel_render: the workgroups of a table walk at most, 0 = VRENDER_MAX_GROUPS
std::atomic<int> g_stages{0};  // and the kernels a call enqueues, 0 = all

}  // namespace

extern "C" {

int sv_voxel_render_device(const void *map, size_t map_bytes, const sv_voxel_map_spec *spec, const sv_voxel_render_spec *cam, const double *cams, int views,
                           int64_t min_n, int64_t min_rows, int since, int32_t *depth, int64_t *key, uint8_t *color, float *disparity, const float *measured,
                           const double *tol, uint8_t *label, int64_t *stats, int64_t *counts, void *stream) {
    int nc[3], l;
    if (const char *bad = check_voxel_map("sv_voxel_render", map, map_bytes, spec, nc, &l)) return refuse(bad);
    if (!cam) return refuse("sv_voxel_render: cam is NULL");
    for (int k = 0; k < 5; k++)
        if (cam->reserved[k] != 0) return refuse("sv_voxel_render: a reserved word of cam is not 0");
    if (views < 0 || views > sv::VRENDER_VIEWS_MAX) return refuse("sv_voxel_render: views outside 0..4096");
    if (cam->width < 1 || cam->width > sv::VRENDER_SIDE_MAX || cam->height < 1 || cam->height > sv::VRENDER_SIDE_MAX)
        return refuse("sv_voxel_render: width or height outside 1..8192");
    if ((int64_t)views * cam->width * cam->height >= ((int64_t)1 << 31)) return refuse("sv_voxel_render: views * width * height >= 2^31");
    const double words[8] = {cam->f, cam->cx, cam->cy, cam->q32, cam->q33, cam->half_px, cam->near, cam->far};
    for (int k = 0; k < 8; k++)
        if (!isfinite(words[k])) return refuse("sv_voxel_render: f, cx, cy, q32, q33, half_px, near or far of cam is not finite");
    if (!(cam->f > 0.0) || cam->q32 == 0.0) return refuse("sv_voxel_render: cam needs f > 0 and q32 != 0");
    if (cam->half_px < 0.0) return refuse("sv_voxel_render: half_px < 0");
    if (cam->r_max < 0 || cam->r_max > sv::VRENDER_R_MAX) return refuse("sv_voxel_render: r_max outside 0..8");
    if (!(0.0 < cam->near && cam->near < cam->far && cam->far <= 1048576.0)) return refuse("sv_voxel_render: near and far need 0 < near < far <= 2^20");
    if (min_n < 1) return refuse("sv_voxel_render: min_n < 1");
    if (measured ? !(label && counts) : (label || counts)) return refuse("sv_voxel_render: measured, label and counts go together");
    if (measured && (!tol || !(*tol >= 0.0))) return refuse("sv_voxel_render: tol is NULL, negative or NaN");
    if (views > 0 && (!cams || !depth || !key || !stats)) return refuse("sv_voxel_render: cams, depth, key or stats is NULL");
    if (any_misaligned(8, cams, key, stats, counts)) return refuse("sv_voxel_render: cams, key, stats or counts is not 8-byte aligned");
    if (misaligned(depth, 4) || misaligned(color, 4) || misaligned(disparity, 4) || misaligned(measured, 4))
        return refuse("sv_voxel_render: depth, color, disparity or measured is not 4-byte aligned");
    const size_t pixels = (size_t)views * cam->width * cam->height;
    const Span spans[] = {{map, map_bytes}, {cams, (size_t)views * 12 * sizeof(double)}, {measured, pixels * 4}, {depth, pixels * 4}, {key, pixels * 8},
                          {color, pixels * 4}, {disparity, pixels * 4}, {label, pixels}, {stats, (size_t)views * 2 * sizeof(int64_t)},
                          {counts, (size_t)views * sv::VRENDER_LABELS * sizeof(int64_t)}};
    if (outputs_overlap(spans, 10, 3)) return refuse("sv_voxel_render: an output shares a byte with the map, cams, measured or another output");
    if (views == 0) return SV_OK;  // nothing to enqueue

    sv::VoxelRenderArgs a;
    memset(&a, 0, sizeof(a));
    a.map = static_cast<const uint8_t *>(map);
    a.log2_slots = l, a.size = spec->size;
    for (int k = 0; k < 3; k++) a.lo[k] = spec->lo[k];
    a.min_n = min_n, a.min_rows = min_rows, a.since = since;
    a.f = cam->f, a.cx = cam->cx, a.cy = cam->cy, a.q32 = cam->q32, a.q33 = cam->q33, a.half_px = cam->half_px, a.near = cam->near, a.far = cam->far;
    a.width = cam->width, a.height = cam->height, a.r_max = cam->r_max, a.views = views;
    a.cams = cams;
    a.depth = reinterpret_cast<uint32_t *>(depth), a.key = reinterpret_cast<unsigned long long *>(key), a.color = color, a.disparity = disparity;
    a.measured = measured, a.tol = measured ? *tol : 0.0, a.label = label;
    a.stats = reinterpret_cast<long long *>(stats), a.counts = reinterpret_cast<long long *>(counts);
    const int groups = g_groups.load();
    if (sv::launch_voxel_render(a, groups ? groups : sv::VRENDER_MAX_GROUPS, g_stages.load(), static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_voxel_render: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_voxel_render(int groups, int stages) {
    if (stages >= 0 && stages <= 3) g_stages.store(stages);
    if (groups < 0 || groups > sv::VRENDER_MAX_GROUPS) return g_groups.load();
    return g_groups.exchange(groups);
}

} /* extern "C" */
