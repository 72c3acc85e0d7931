// Group (F) of include/stereo_vision_hip.h: compact coloured point clouds from disparity maps (cloud_kernels.hip).  Everything here is
// argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its text for
// sv_last_error(NULL).
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "cloud_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

// NULL for a good spec and good sizes, else what is wrong with them.
const char *check_shape(const sv_cloud_spec *s, int batch, int width, int height) {
    if (!s) return "sv_cloud: spec is NULL";
    for (int k = 0; k < 5; k++)
        if (s->reserved[k] != 0) return "sv_cloud: a reserved word of the spec is not 0";
    if (s->disparity != SV_CLOUD_DMAP && s->disparity != SV_CLOUD_D1) return "sv_cloud: disparity is not SV_CLOUD_DMAP / SV_CLOUD_D1";
    if (s->dtype != SV_CLOUD_F32 && s->dtype != SV_CLOUD_F64) return "sv_cloud: dtype is not SV_CLOUD_F32 / SV_CLOUD_F64";
    if (s->step < 1) return "sv_cloud: step < 1";
    for (int k = 0; k < 3; k++)
        if (!(s->lo[k] < s->hi[k])) return "sv_cloud: the crop needs lo < hi on every axis (NaN is refused)";
    return check_frame("sv_cloud", batch, width, height, 0);
}

// The visited lattice of a checked shape.
void lattice(const sv_cloud_spec *s, int width, int height, int *Wv, int *n_visited, int *n_tiles) {
    const int64_t wv = ((int64_t)width + s->step - 1) / s->step, hv = ((int64_t)height + s->step - 1) / s->step;
    *Wv = (int)wv;
    *n_visited = (int)(wv * hv);  // <= width * height < 2^31
    *n_tiles = (int)((wv * hv + sv::CLOUD_TILE - 1) / sv::CLOUD_TILE);
}

}  // namespace

extern "C" {

int sv_cloud_tile(void) { return sv::CLOUD_TILE; }

size_t sv_cloud_workspace_bytes(const sv_cloud_spec *spec, int batch, int width, int height) {
    if (check_shape(spec, batch, width, height)) return SIZE_MAX;
    int Wv, n_visited, n_tiles;
    lattice(spec, width, height, &Wv, &n_visited, &n_tiles);
    return (size_t)batch * n_tiles * sizeof(int32_t);
}

int sv_cloud_disparity_device(const float *disp, const uint8_t *colors, int batch, int width, int height, const double *Q16, const double *XR9,
                              const double *XT3, const sv_cloud_spec *spec, int capacity, void *xyz, uint8_t *color_out, int32_t *index_out, int32_t *counts,
                              void *workspace, size_t workspace_bytes, void *stream) {
    if (const char *bad = check_shape(spec, batch, width, height)) return refuse(bad);
    if (!disp) return refuse("sv_cloud: disp is NULL");
    if (!Q16) return refuse("sv_cloud: Q16 is NULL");
    if (!counts) return refuse("sv_cloud: counts is NULL");
    if (capacity < 0) return refuse("sv_cloud: capacity < 0");
    if (capacity > 0 && !xyz) return refuse("sv_cloud: xyz is NULL with capacity > 0");
    if (color_out && !colors) return refuse("sv_cloud: color_out without colors");
    if ((reinterpret_cast<uintptr_t>(colors) | reinterpret_cast<uintptr_t>(color_out)) & 3) return refuse("sv_cloud: colors / color_out are not 4-byte aligned");
    const size_t need = sv_cloud_workspace_bytes(spec, batch, width, height);
    if (need > 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 3)))
        return refuse("sv_cloud: the workspace is NULL, misaligned or smaller than sv_cloud_workspace_bytes");
    if (batch == 0) return SV_OK;

    sv::CloudArgs a;
    memset(&a, 0, sizeof(a));
    set_reproject(a.rp, Q16, XR9, XT3);
    for (int k = 0; k < 3; k++) a.lo[k] = spec->lo[k], a.hi[k] = spec->hi[k];
    a.disp = disp, a.colors = colors;
    a.xyz = xyz, a.color_out = color_out, a.index_out = index_out, a.counts = counts;
    a.tiles = static_cast<int32_t *>(workspace);
    a.W = width, a.H = height, a.step = spec->step, a.capacity = capacity;
    lattice(spec, width, height, &a.Wv, &a.n_visited, &a.n_tiles);

    hipStream_t st = static_cast<hipStream_t>(stream);
    if (sv::launch_cloud_count(spec->disparity, a, batch, st) != hipSuccess || sv::launch_cloud_scan(a, batch, st) != hipSuccess ||
        (capacity > 0 && sv::launch_cloud_write(spec->disparity, spec->dtype, a, batch, st) != hipSuccess)) {
        sv_internal_set_error("sv_cloud: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
