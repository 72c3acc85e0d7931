// Group (AA) of include/stereo_vision_hip.h: the previous frame's disparity map warped into the current frame (warp_kernels.hip).
// Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a refused call leaves its
// text for sv_last_error(NULL).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "warp_kernels.h"

namespace {

using namespace sv::glue;

// NULL for a spec the kernels can use, else what is wrong with it.
const char *check_spec(const char *prefix, const sv_warp_spec *s) {
    if (!s) return prefixed(prefix, "spec is NULL");
    for (int k = 0; k < 12; k++)
        if (s->reserved[k] != 0) return prefixed(prefix, "a reserved word of the spec is not 0");
    if (const char *bad = check_camera_words(prefix, s)) return bad;
    if (s->e_max < 0 || s->e_max > sv::WARP_E_MAX) return prefixed(prefix, "e_max outside 0..4");
    if (s->tol_q < 0 || s->tol_q > sv::WARP_TOL_MAX) return prefixed(prefix, "tol_q outside 0..2^20");
    if (s->rel_q < 0 || s->rel_q > sv::WARP_REL_MAX) return prefixed(prefix, "rel_q outside 0..256");
    if (s->mode < sv::WARP_MODE_FILL || s->mode > sv::WARP_MODE_REJECT) return prefixed(prefix, "mode outside 0..2");
    return nullptr;
}

}  // namespace

extern "C" {

int sv_disparity_warp_workspace(int width, int height, int batch, size_t *bytes) {
    if (!bytes) return refuse("sv_disparity_warp_workspace: bytes is NULL");
    if (const char *bad = check_images("sv_disparity_warp_workspace", batch, width, height)) return refuse(bad);
    *bytes = (size_t)batch * (size_t)width * (size_t)height * sizeof(unsigned long long);
    return SV_OK;
}

int sv_disparity_warp_device(const float *d_prev, const float *d_cur, const double *poses, int batch, int width, int height, const sv_warp_spec *spec,
                             int32_t *expected, int32_t *source, uint8_t *label, float *out, int32_t *counts, void *workspace, size_t workspace_bytes,
                             void *stream) {
    if (const char *bad = check_images("sv_disparity_warp", batch, width, height)) return refuse(bad);
    if (const char *bad = check_spec("sv_disparity_warp", spec)) return refuse(bad);
    if (batch > 0 && (!d_prev || !poses)) return refuse("sv_disparity_warp: d_prev or poses is NULL");
    if (batch > 0 && (!expected || !source || !counts)) return refuse("sv_disparity_warp: expected, source or counts is NULL");
    if (batch > 0 && d_cur && (!label || !out)) return refuse("sv_disparity_warp: label or out is NULL beside a d_cur");
    if (any_misaligned(4, d_prev, d_cur, out) || any_misaligned(4, expected, source, counts))
        return refuse("sv_disparity_warp: d_prev, d_cur, expected, source, out or counts is not 4-byte aligned");
    if (misaligned(poses, 8)) return refuse("sv_disparity_warp: poses is not 8-byte aligned");
    size_t need;
    sv_disparity_warp_workspace(width, height, batch, &need);
    if (batch > 0 && !workspace) return refuse("sv_disparity_warp: the workspace is NULL");
    if (misaligned(workspace, 8)) return refuse("sv_disparity_warp: the workspace is not 8-byte aligned");
    if (workspace_bytes < need) return refuse("sv_disparity_warp: the workspace is smaller than sv_disparity_warp_workspace asks for");
    const size_t px = (size_t)batch * (size_t)width * (size_t)height;
    const size_t with_cur = d_cur ? px : 0;
    const Span spans[] = {{d_prev, px * 4}, {d_cur, with_cur * 4}, {poses, (size_t)batch * 12 * 8}, {workspace, need}, {expected, px * 4},
                          {source, px * 4}, {label, with_cur}, {out, with_cur * 4}, {counts, (size_t)batch * sv::WARP_COUNT_WORDS * 4}};
    if (outputs_overlap(spans, 9, 3)) return refuse("sv_disparity_warp: an output or the workspace shares bytes with an input or another output");
    if (batch == 0) return SV_OK;  // nothing to do

    sv::WarpArgs a;
    memset(&a, 0, sizeof(a));
    a.d_prev = d_prev, a.d_cur = d_cur, a.poses = poses;
    a.cam = sv::FlowCamera{spec->f, spec->cx, spec->cy, spec->b16, spec->fb, spec->fb16};
    a.B = batch, a.H = height, a.W = width;
    a.e_max = spec->e_max, a.tol_q = spec->tol_q, a.rel_q = spec->rel_q, a.mode = spec->mode;
    a.keys = static_cast<unsigned long long *>(workspace);
    a.expected = expected, a.source = source, a.label = label, a.out = out, a.counts = counts;
    if (sv::launch_disparity_warp(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_disparity_warp: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
