// Group (J) of include/stereo_vision_hip.h: occupancy and elevation grids from disparity maps, obstacle labels and free space
// (occupancy_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a
// refused call leaves its text for sv_last_error(NULL).
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "occupancy_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_combine{1};
std::atomic<unsigned long long *> g_atomics{nullptr};

// NULL for a good spec, else what is wrong with it; the grid comes from the top view's own checks.
const char *check_spec(const sv_occupancy_spec *s, int *rows, int *cols) {
    if (!s) return "sv_occupancy: spec is NULL";
    for (int k = 0; k < 5; k++)
        if (s->reserved[k] != 0) return "sv_occupancy: a reserved word of the spec is not 0";
    sv_top_view_spec tv;
    memset(&tv, 0, sizeof(tv));
    memcpy(tv.x_range, s->x_range, sizeof(tv.x_range));
    memcpy(tv.y_range, s->y_range, sizeof(tv.y_range));
    memcpy(tv.z_range, s->z_range, sizeof(tv.z_range));
    tv.scale = s->scale, tv.mode = SV_TOPVIEW_COUNT, tv.disparity = SV_TOPVIEW_D1;
    if (sv_top_view_dims(&tv, rows, cols) != SV_OK) return "sv_occupancy: the ranges or the scale are not a grid sv_top_view_dims admits";
    if (s->z_scale < 1 || s->z_scale > 65536) return "sv_occupancy: z_scale outside 1..65536";
    if (s->min_obstacle < 1 || s->min_ground < 1 || s->min_rays < 1) return "sv_occupancy: min_obstacle, min_ground or min_rays < 1";
    return nullptr;
}

}  // namespace

extern "C" {

int sv_occupancy_dims(const sv_occupancy_spec *spec, int *rows, int *cols) {
    int r, c;
    if (!rows || !cols) return refuse("sv_occupancy: rows or cols is NULL");
    if (const char *bad = check_spec(spec, &r, &c)) return refuse(bad);
    *rows = r;
    *cols = c;
    return SV_OK;
}

int sv_occupancy_disparity_device(const float *disp, const uint8_t *labels, const int32_t *free_row, const float *free_disp, int batch, int width, int height,
                                  const double *Q16, const double *XR9, const double *XT3, const sv_occupancy_spec *spec, int32_t *cells, int32_t *n_rays,
                                  uint8_t *state, void *stream) {
    int rows, cols;
    if (const char *bad = check_spec(spec, &rows, &cols)) return refuse(bad);
    if (const char *bad = check_frame("sv_occupancy", batch, width, height, 32768)) return refuse(bad);
    if (!disp || !labels || !free_row || !free_disp) return refuse("sv_occupancy: disp, labels, free_row or free_disp is NULL");
    if (!Q16) return refuse("sv_occupancy: Q16 is NULL");
    if (!cells || !n_rays) return refuse("sv_occupancy: cells or n_rays is NULL");
    if ((reinterpret_cast<uintptr_t>(disp) | reinterpret_cast<uintptr_t>(free_row) | reinterpret_cast<uintptr_t>(free_disp) | reinterpret_cast<uintptr_t>(n_rays)) & 3)
        return refuse("sv_occupancy: disp, free_row, free_disp or n_rays is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(cells) & 15) return refuse("sv_occupancy: cells is not 16-byte aligned (a cell is stored as one 16-byte word)");
    const double s = (double)spec->scale;
    const double ox = XT3 ? XT3[0] * s : 0.0, oy = XT3 ? XT3[1] * s : 0.0;
    if (!(fabs(ox) < (double)sv::OCC_CELL_MAX && fabs(oy) < (double)sv::OCC_CELL_MAX))  // NaN fails too
        return refuse("sv_occupancy: the origin of the sight lines (XT3) lies 2^24 cells or more from the frame's origin");
    if (batch == 0) return SV_OK;

    sv::OccupancyArgs a;
    memset(&a, 0, sizeof(a));
    set_reproject(a.rp, Q16, XR9, XT3);
    a.disp = disp, a.labels = labels, a.free_row = free_row, a.free_disp = free_disp;
    a.cells = cells, a.n_rays = n_rays, a.state = state;
    a.atomics = g_atomics.load();
    a.W = width, a.H = height, a.rows = rows, a.cols = cols;
    a.x0 = spec->x_range[0], a.x1 = spec->x_range[1];
    a.y0 = spec->y_range[0], a.y1 = spec->y_range[1];
    a.z0 = spec->z_range[0], a.z1 = spec->z_range[1];
    a.s = s, a.zs = (double)spec->z_scale;
    a.x1s = trunc(a.x1 * a.s), a.y1s = trunc(a.y1 * a.s);  // |.| <= 2^46: exact
    a.r0 = (long long)(a.x1s - trunc(ox)), a.c0 = (long long)(a.y1s - trunc(oy));
    a.min_obstacle = spec->min_obstacle, a.min_ground = spec->min_ground, a.min_rays = spec->min_rays;

    // SV_OCCUPANCY_STAGE = clear, evidence or rays leaves out the kernels behind that stage (tools/occupancy_time.py times the
    // prefixes); the outputs are then unfinished
    const char *stage = getenv("SV_OCCUPANCY_STAGE");
    const int last = !stage ? 3 : strcmp(stage, "clear") == 0 ? 0 : strcmp(stage, "evidence") == 0 ? 1 : strcmp(stage, "rays") == 0 ? 2 : 3;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (sv::launch_occupancy_clear(a, batch, st) != hipSuccess ||
        (last >= 1 && sv::launch_occupancy_evidence(a, batch, g_combine.load() != 0, st) != hipSuccess) ||
        (last >= 2 && sv::launch_occupancy_rays(a, batch, st) != hipSuccess) || (last >= 3 && sv::launch_occupancy_finalize(a, batch, st) != hipSuccess)) {
        sv_internal_set_error("sv_occupancy: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_occupancy(int combine, unsigned long long *atomics_device) {
    g_combine.store(combine != 0 ? 1 : 0);
    g_atomics.store(atomics_device);
    return SV_OK;
}

} /* extern "C" */
