// Group (G) of include/stereo_vision_hip.h: ground plane, obstacle labels and free space from disparity maps (ground_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "ground_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

// NULL for a good spec and good sizes, else what is wrong with them.
const char *check_shape(const sv_ground_spec *s, int batch, int width, int height) {
    if (!s) return "sv_ground: spec is NULL";
    for (int k = 0; k < 7; k++)
        if (s->reserved[k] != 0) return "sv_ground: a reserved word of the spec is not 0";
    if (const char *bad = check_frame("sv_ground", batch, width, height, 32768)) return bad;
    if (s->n_bins < 8 || s->n_bins > sv::GROUND_BINS_MAX) return "sv_ground: n_bins outside 8..4096";
    if (s->vh_lo < -32768 || s->vh_lo > s->vh_hi || s->vh_hi > height - 2) return "sv_ground: the horizon rows need -32768 <= vh_lo <= vh_hi <= height - 2";
    if (s->vh_step < 1) return "sv_ground: vh_step < 1";
    if (s->qb_step < 1 || s->qb_step >= s->n_bins) return "sv_ground: qb_step outside 1..n_bins - 1";
    if (s->tol < 0 || s->tol > 16) return "sv_ground: tol outside 0..16";
    if (s->g_tol < 0 || s->g_tol > 4096) return "sv_ground: g_tol outside 0..4096";
    if (s->min_run < 1) return "sv_ground: min_run < 1";
    if (s->min_support < 0) return "sv_ground: min_support < 0";
    return nullptr;
}

int horizon_rows(const sv_ground_spec *s) { return (s->vh_hi - s->vh_lo) / s->vh_step + 1; }  // <= 2^16

size_t key_bytes(const sv_ground_spec *s, int batch) { return (size_t)batch * horizon_rows(s) * sizeof(uint64_t); }

}  // namespace

extern "C" {

size_t sv_ground_workspace_bytes(const sv_ground_spec *spec, int batch, int width, int height) {
    if (check_shape(spec, batch, width, height)) return SIZE_MAX;
    return key_bytes(spec, batch) + (size_t)batch * height * (spec->n_bins + 1) * sizeof(uint32_t);
}

int sv_ground_disparity_device(const float *disp, int batch, int width, int height, const sv_ground_spec *spec, uint32_t *vdisp, int32_t *ground,
                               uint8_t *labels, int32_t *free_row, float *free_disp, void *workspace, size_t workspace_bytes, void *stream) {
    if (const char *bad = check_shape(spec, batch, width, height)) return refuse(bad);
    if (!disp) return refuse("sv_ground: disp is NULL");
    if (!ground) return refuse("sv_ground: ground is NULL");
    if ((reinterpret_cast<uintptr_t>(disp) | reinterpret_cast<uintptr_t>(vdisp) | reinterpret_cast<uintptr_t>(ground) | reinterpret_cast<uintptr_t>(free_row) |
         reinterpret_cast<uintptr_t>(free_disp)) & 3)
        return refuse("sv_ground: disp, vdisp, ground, free_row or free_disp is not 4-byte aligned");
    const size_t need = sv_ground_workspace_bytes(spec, batch, width, height);
    if (need > 0 && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 7)))
        return refuse("sv_ground: the workspace is NULL, not 8-byte aligned or smaller than sv_ground_workspace_bytes");
    if (batch == 0) return SV_OK;

    sv::GroundArgs a;
    memset(&a, 0, sizeof(a));
    a.disp = disp, a.vdisp = vdisp, a.ground = ground, a.labels = labels, a.free_row = free_row, a.free_disp = free_disp;
    a.keys = static_cast<uint64_t *>(workspace);
    a.prefix = reinterpret_cast<uint32_t *>(static_cast<char *>(workspace) + key_bytes(spec, batch));
    a.W = width, a.H = height, a.n_bins = spec->n_bins;
    a.vh_lo = spec->vh_lo, a.vh_step = spec->vh_step, a.n_vh = horizon_rows(spec);
    a.qb_step = spec->qb_step, a.n_qb = (spec->n_bins - 1) / spec->qb_step;  // qb_step, 2 qb_step, ... < n_bins: at least one
    a.tol = spec->tol, a.g_tol = spec->g_tol, a.min_run = spec->min_run, a.min_support = spec->min_support;

    // SV_GROUND_HIST=plain: one LDS atomic per pixel instead of one per run of equal bins (tools/ground_time.py measures both); the
    // counts are the same
    const char *hist = getenv("SV_GROUND_HIST");
    const bool aggregate = !(hist && strcmp(hist, "plain") == 0);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (sv::launch_ground_hist(a, batch, aggregate, st) != hipSuccess || sv::launch_ground_search(a, batch, st) != hipSuccess ||
        sv::launch_ground_pick(a, batch, st) != hipSuccess ||
        ((labels || free_row || free_disp) && sv::launch_ground_label(a, batch, st) != hipSuccess)) {
        sv_internal_set_error("sv_ground: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
