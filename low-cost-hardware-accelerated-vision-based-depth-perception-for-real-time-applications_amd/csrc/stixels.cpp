// Group (H) of include/stereo_vision_hip.h: stixels and detector-free object boxes from disparity maps and obstacle labels
// (stixel_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a
// refused call leaves its text for sv_last_error(NULL).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "stixel_kernels.h"

namespace {

using namespace sv::glue;

// NULL for a good spec and good sizes, else what is wrong with them.
const char *check_shape(const sv_stixel_spec *s, int batch, int width, int height) {
    if (!s) return "sv_stixel: spec is NULL";
    for (int k = 0; k < 7; k++)
        if (s->reserved[k] != 0) return "sv_stixel: a reserved word of the spec is not 0";
    if (const char *bad = check_frame("sv_stixel", batch, width, height, 32768)) return bad;
    if (s->n_bins < 8 || s->n_bins > 4096) return "sv_stixel: n_bins outside 8..4096";
    if (s->q_min < 0 || s->q_min > 4095) return "sv_stixel: q_min outside 0..4095";
    if (s->sim < 0 || s->sim > 4096) return "sv_stixel: sim outside 0..4096";
    if (s->max_gap < 0 || s->max_gap > 255) return "sv_stixel: max_gap outside 0..255";
    if (s->min_rows < 1) return "sv_stixel: min_rows < 1";
    if (s->max_layers < 1 || s->max_layers > 64) return "sv_stixel: max_layers outside 1..64";
    if (s->col_step < 1) return "sv_stixel: col_step < 1";
    if (s->sim_cols < 0 || s->sim_cols > 4096) return "sv_stixel: sim_cols outside 0..4096";
    if (s->min_cols < 1) return "sv_stixel: min_cols < 1";
    return nullptr;
}

int visited_columns(const sv_stixel_spec *s, int width) { return (width - 1) / s->col_step + 1; }  // ceil(width / col_step), no overflow

}  // namespace

extern "C" {

size_t sv_stixel_workspace_bytes(const sv_stixel_spec *spec, int batch, int width, int height) {
    if (check_shape(spec, batch, width, height)) return SIZE_MAX;
    return (size_t)batch * visited_columns(spec, width) * sizeof(int4);
}

int sv_stixel_disparity_device(const float *disp, const uint8_t *labels, int batch, int width, int height, const sv_stixel_spec *spec, int capacity,
                               int32_t *stixels, int32_t *n_stixels, int32_t *boxes, int32_t *info, int32_t *counts, void *workspace,
                               size_t workspace_bytes, void *stream) {
    if (const char *bad = check_shape(spec, batch, width, height)) return refuse(bad);
    if (!disp) return refuse("sv_stixel: disp is NULL");
    if (!labels) return refuse("sv_stixel: labels is NULL");
    if (!counts) return refuse("sv_stixel: counts is NULL");
    if (capacity < 0) return refuse("sv_stixel: capacity < 0");
    if ((reinterpret_cast<uintptr_t>(disp) | reinterpret_cast<uintptr_t>(n_stixels) | reinterpret_cast<uintptr_t>(counts)) & 3)
        return refuse("sv_stixel: disp, n_stixels or counts is not 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(stixels) | reinterpret_cast<uintptr_t>(boxes) | reinterpret_cast<uintptr_t>(info)) & 15)
        return refuse("sv_stixel: stixels, boxes or info is not 16-byte aligned");
    const size_t need = sv_stixel_workspace_bytes(spec, batch, width, height);
    if (need > 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)))
        return refuse("sv_stixel: the workspace is NULL, not 16-byte aligned or smaller than sv_stixel_workspace_bytes");
    if (batch == 0) return SV_OK;

    sv::StixelArgs a;
    memset(&a, 0, sizeof(a));
    a.disp = disp, a.labels = labels, a.n_stixels = n_stixels, a.counts = counts;
    a.stixels = reinterpret_cast<int4 *>(stixels), a.boxes = reinterpret_cast<int4 *>(boxes), a.info = reinterpret_cast<int4 *>(info);
    a.layer0 = static_cast<int4 *>(workspace);
    a.W = width, a.H = height, a.Wv = visited_columns(spec, width);
    a.n_bins = spec->n_bins, a.q_min = spec->q_min, a.sim = spec->sim, a.max_gap = spec->max_gap, a.min_rows = spec->min_rows;
    a.max_layers = spec->max_layers, a.col_step = spec->col_step, a.sim_cols = spec->sim_cols, a.min_cols = spec->min_cols;
    a.capacity = capacity;

    // SV_STIXEL_STAGE=columns: the first kernel alone (tools/stixel_time.py times it); boxes, info and counts are then not written
    const char *stage = getenv("SV_STIXEL_STAGE");
    const bool objects = !(stage && strcmp(stage, "columns") == 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (sv::launch_stixel_columns(a, batch, st) != hipSuccess || (objects && sv::launch_stixel_objects(a, batch, st) != hipSuccess)) {
        sv_internal_set_error("sv_stixel: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
