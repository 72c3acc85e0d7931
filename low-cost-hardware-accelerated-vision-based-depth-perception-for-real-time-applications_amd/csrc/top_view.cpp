// Group (D) of include/stereo_vision_hip.h: bird's-eye views of point clouds or disparity maps (top_view_kernels.hip).  Everything
// here is argument checking and launch set-up; every check runs before anything is enqueued.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "top_view_kernels.h"

namespace {

std::atomic<int> g_combine{1};
std::atomic<unsigned long long *> g_atomics{nullptr};

const double kMaxBound = 2147483648.0;  // |x|, |y| <= 2^31: with scale <= 32767, x * scale stays an exact double
const int kMaxDim = 32768;

bool integer_bound(double v) { return isfinite(v) && v == trunc(v) && fabs(v) <= kMaxBound; }

// The grid of a valid spec; false for a bad one.
bool grid_of(const sv_top_view_spec *s, int *rows, int *cols) {
    if (!s) return false;
    for (int k = 0; k < 5; k++)
        if (s->reserved[k] != 0) return false;
    if (s->scale < 1 || (s->mode != SV_TOPVIEW_REFERENCE && s->mode != SV_TOPVIEW_COUNT) || (s->disparity != SV_TOPVIEW_DMAP && s->disparity != SV_TOPVIEW_D1))
        return false;
    const double *xr = s->x_range, *yr = s->y_range, *zr = s->z_range;
    if (!integer_bound(xr[0]) || !integer_bound(xr[1]) || !integer_bound(yr[0]) || !integer_bound(yr[1])) return false;
    if (!(xr[0] < xr[1]) || !(yr[0] < yr[1]) || !(zr[0] < zr[1])) return false;  // NaN fails too
    const double r = (xr[1] - xr[0]) * s->scale + 1, c = (yr[1] - yr[0]) * s->scale + 1;
    if (r > kMaxDim || c > kMaxDim) return false;
    if (s->mode == SV_TOPVIEW_REFERENCE && xr[1] == 0 && yr[1] == 0) return false;  // max_dist == 0
    *rows = (int)r;
    *cols = (int)c;
    return true;
}

sv::TopViewArgs base_args(const sv_top_view_spec *s, int rows, int cols, void *grid) {
    sv::TopViewArgs a;
    memset(&a, 0, sizeof(a));
    a.grid = grid;
    a.atomics = g_atomics.load();
    a.rows = rows, a.cols = cols;
    a.x0 = s->x_range[0], a.x1 = s->x_range[1];
    a.y0 = s->y_range[0], a.y1 = s->y_range[1];
    a.z0 = s->z_range[0], a.z1 = s->z_range[1];
    a.s = (double)s->scale;
    a.x1s = trunc(a.x1 * a.s), a.y1s = trunc(a.y1 * a.s);
    a.max_dist = sqrt(a.x1 * a.x1 + a.y1 * a.y1);  // -ffp-contract=off: as numpy computes it
    return a;
}

// Zero the grid (count) or the keys (reference), rasterise, finalize.
int run(int src, const sv_top_view_spec *s, int batch, int rows, int cols, sv::TopViewArgs &a, void *out, void *workspace, hipStream_t st) {
    const size_t cells = (size_t)batch * rows * cols;
    const bool ref = s->mode == SV_TOPVIEW_REFERENCE;
    if (hipMemsetAsync(ref ? workspace : out, 0, cells * (ref ? 8 : 4), st) != hipSuccess) return SV_ERR_HIP;
    if ((size_t)a.W * a.H > 0 && sv::launch_top_view(src, s->mode, g_combine.load() != 0, a, batch, st) != hipSuccess) return SV_ERR_HIP;
    if (ref && sv::launch_top_view_finalize(static_cast<const uint64_t *>(workspace), static_cast<uint8_t *>(out), cells, st) != hipSuccess) return SV_ERR_HIP;
    return SV_OK;
}

// Buffers of a call: out always, the workspace in reference mode (large enough, 8-byte aligned).
bool buffers_ok(const sv_top_view_spec *s, int batch, const void *out, const void *workspace, size_t workspace_bytes) {
    if (!out) return false;
    if (s->mode != SV_TOPVIEW_REFERENCE) return true;
    return workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= sv_top_view_workspace_bytes(s, batch);
}

}  // namespace

extern "C" {

int sv_top_view_dims(const sv_top_view_spec *spec, int *rows, int *cols) {
    int r, c;
    if (!rows || !cols || !grid_of(spec, &r, &c)) return SV_ERR_ARG;
    *rows = r;
    *cols = c;
    return SV_OK;
}

size_t sv_top_view_workspace_bytes(const sv_top_view_spec *spec, int batch) {
    int r, c;
    if (batch < 0 || !grid_of(spec, &r, &c)) return SIZE_MAX;
    return spec->mode == SV_TOPVIEW_REFERENCE ? (size_t)batch * r * c * sizeof(uint64_t) : 0;
}

int sv_top_view_points_device(const double *points, int batch, int64_t n_points, const sv_top_view_spec *spec, void *out, void *workspace,
                              size_t workspace_bytes, void *stream) {
    int rows, cols;
    if (!grid_of(spec, &rows, &cols) || !points || batch < 0 || batch > 65535 || n_points < 0 || n_points >= ((int64_t)1 << 31)) return SV_ERR_ARG;
    if (!buffers_ok(spec, batch, out, workspace, workspace_bytes)) return SV_ERR_ARG;
    if (batch == 0) return SV_OK;
    sv::TopViewArgs a = base_args(spec, rows, cols, spec->mode == SV_TOPVIEW_REFERENCE ? workspace : out);
    a.points = points;
    a.W = (int)n_points, a.H = 1;
    return run(sv::TV_SRC_POINTS, spec, batch, rows, cols, a, out, workspace, static_cast<hipStream_t>(stream));
}

int sv_top_view_disparity_device(const float *disp, int batch, int width, int height, const double *Q16, const double *XR9, const double *XT3,
                                 const sv_top_view_spec *spec, void *out, void *workspace, size_t workspace_bytes, void *stream) {
    int rows, cols;
    if (!grid_of(spec, &rows, &cols) || !disp || !Q16 || batch < 0 || batch > 65535 || width < 1 || height < 1 || height > 65535 ||
        (int64_t)width * height >= ((int64_t)1 << 31))
        return SV_ERR_ARG;
    if (!buffers_ok(spec, batch, out, workspace, workspace_bytes)) return SV_ERR_ARG;
    if (batch == 0) return SV_OK;
    sv::TopViewArgs a = base_args(spec, rows, cols, spec->mode == SV_TOPVIEW_REFERENCE ? workspace : out);
    sv::glue::set_reproject(a.rp, Q16, XR9, XT3);
    a.disp = disp;
    a.W = width, a.H = height;
    return run(spec->disparity == SV_TOPVIEW_D1 ? sv::TV_SRC_D1 : sv::TV_SRC_DMAP, spec, batch, rows, cols, a, out, workspace, static_cast<hipStream_t>(stream));
}

int sv_debug_top_view(int combine, unsigned long long *atomics_device) {
    g_combine.store(combine != 0 ? 1 : 0);
    g_atomics.store(atomics_device);
    return SV_OK;
}

} /* extern "C" */
