// Group (Z) of include/stereo_vision_hip.h: the temporal matches of two frames and the sums of one round of the egomotion fit
// (flow_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a
// refused call leaves its text for sv_last_error(NULL).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "flow_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

// NULL for a camera the kernels can use, else what is wrong with it.
const char *check_camera(const char *prefix, const sv_flow_spec *s) {
    if (!s) return prefixed(prefix, "spec is NULL");
    for (int k = 0; k < 9; k++)
        if (s->reserved[k] != 0) return prefixed(prefix, "a reserved word of the spec is not 0");
    return check_camera_words(prefix, s);
}

// NULL for the words of a match call, else what is wrong with them.
const char *check_match_words(const char *prefix, const sv_flow_spec *s) {
    if (const char *bad = check_camera(prefix, s)) return bad;
    if (s->step < 1 || s->step > (1 << 20)) return prefixed(prefix, "step outside 1..2^20");
    if (s->r < 1 || s->r > sv::FLOW_R_MAX) return prefixed(prefix, "r outside 1..7");
    if (s->wx < 0 || s->wx > 8192 || s->wy < 0 || s->wy > 8192) return prefixed(prefix, "wx or wy outside 0..8192");
    if ((2ll * s->wx + 1) * (2ll * s->wy + 1) > sv::FLOW_CANDIDATES_MAX) return prefixed(prefix, "(2 wx + 1) (2 wy + 1) > 16384");
    if (sv::flow_window_bytes(s->r, s->wx, s->wy) > sv::FLOW_WINDOW_BYTES) return prefixed(prefix, "the window takes more than 16384 bytes of LDS");
    if (s->ratio < 0 || s->ratio > 256) return prefixed(prefix, "ratio outside 0..256");
    if (s->max_cost < 0) return prefixed(prefix, "max_cost < 0");
    if (s->capacity < 0 || s->capacity > sv::FLOW_CAPACITY_MAX) return prefixed(prefix, "capacity outside 0..65536");
    return nullptr;
}

long long lattice(int n, int step) { return ((long long)n + step - 1) / step; }

sv::FlowCamera camera_of(const sv_flow_spec *s) { return sv::FlowCamera{s->f, s->cx, s->cy, s->b16, s->fb, s->fb16}; }

int chunks_of(int cap) { return (cap + sv::FLOW_SUM_THREADS - 1) / sv::FLOW_SUM_THREADS; }

}  // namespace

extern "C" {

int sv_flow_match_workspace(int width, int height, int batch, const sv_flow_spec *spec, size_t *bytes) {
    if (!bytes) return refuse("sv_flow_match_workspace: bytes is NULL");
    if (const char *bad = check_images("sv_flow_match_workspace", batch, width, height)) return refuse(bad);
    if (const char *bad = check_match_words("sv_flow_match_workspace", spec)) return refuse(bad);
    *bytes = (size_t)batch * (size_t)(lattice(width, spec->step) * lattice(height, spec->step)) * sv::FLOW_REC_WORDS * sizeof(int32_t);
    return SV_OK;
}

int sv_flow_match_device(const void *prev, const void *cur, const float *d_prev, const float *d_cur, const double *guess, int batch, int width, int height,
                         const sv_flow_spec *spec, int32_t *matches, int32_t *cost, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream) {
    if (const char *bad = check_images("sv_flow_match", batch, width, height)) return refuse(bad);
    if (const char *bad = check_match_words("sv_flow_match", spec)) return refuse(bad);
    if (batch > 0 && (!prev || !cur || !d_prev)) return refuse("sv_flow_match: prev, cur or d_prev is NULL");
    if (batch > 0 && !counts) return refuse("sv_flow_match: counts is NULL");
    if (batch > 0 && spec->capacity > 0 && (!matches || !cost)) return refuse("sv_flow_match: matches or cost is NULL");
    if (any_misaligned(4, d_prev, d_cur) || any_misaligned(4, matches, cost, counts)) return refuse("sv_flow_match: d_prev, d_cur, matches, cost or counts is not 4-byte aligned");
    if (misaligned(guess, 8)) return refuse("sv_flow_match: guess is not 8-byte aligned");
    size_t need;
    sv_flow_match_workspace(width, height, batch, spec, &need);
    if (batch > 0 && !workspace) return refuse("sv_flow_match: the workspace is NULL");
    if (misaligned(workspace, 4)) return refuse("sv_flow_match: the workspace is not 4-byte aligned");
    if (workspace_bytes < need) return refuse("sv_flow_match: the workspace is smaller than sv_flow_match_workspace asks for");
    if (batch == 0) return SV_OK;  // nothing to do

    sv::FlowMatchArgs a;
    memset(&a, 0, sizeof(a));
    a.prev = static_cast<const uint8_t *>(prev), a.cur = static_cast<const uint8_t *>(cur);
    a.d_prev = d_prev, a.d_cur = d_cur, a.guess = guess;
    a.cam = camera_of(spec);
    a.B = batch, a.H = height, a.W = width;
    a.step = spec->step, a.r = spec->r, a.wx = spec->wx, a.wy = spec->wy, a.ratio = spec->ratio, a.max_cost = spec->max_cost, a.capacity = spec->capacity;
    a.nlx = (int)lattice(width, spec->step), a.nly = (int)lattice(height, spec->step);
    a.pitch = sv::flow_pitch(spec->r, spec->wx), a.rows = 2 * spec->wy + 2 * spec->r + 1;
    a.rec = static_cast<int32_t *>(workspace);
    a.matches = matches, a.cost = cost, a.counts = counts;
    if (sv::launch_flow_match(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_flow_match: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_flow_pose_sums_workspace(int capacity, int batch, size_t *bytes) {
    if (!bytes) return refuse("sv_flow_pose_sums_workspace: bytes is NULL");
    if (capacity < 0 || capacity > sv::FLOW_CAPACITY_MAX) return refuse("sv_flow_pose_sums_workspace: capacity outside 0..65536");
    if (batch < 0 || batch > 65535) return refuse("sv_flow_pose_sums_workspace: batch outside 0..65535");
    *bytes = (size_t)batch * chunks_of(capacity) * sv::FLOW_SUM_WORDS * sizeof(unsigned long long);
    return SV_OK;
}

int sv_flow_pose_sums_device(const int32_t *matches, const int32_t *counts, const double *poses, int batch, int capacity, const sv_flow_spec *spec, int gate_q,
                             int dgate_q, int64_t *sums, void *workspace, size_t workspace_bytes, void *stream) {
    if (const char *bad = check_camera("sv_flow_pose_sums", spec)) return refuse(bad);
    if (capacity < 0 || capacity > sv::FLOW_CAPACITY_MAX) return refuse("sv_flow_pose_sums: capacity outside 0..65536");
    if (batch < 0 || batch > 65535) return refuse("sv_flow_pose_sums: batch outside 0..65535");
    if (gate_q < 0 || gate_q > sv::FLOW_GATE_MAX || dgate_q < 0 || dgate_q > sv::FLOW_GATE_MAX) return refuse("sv_flow_pose_sums: gate_q or dgate_q outside 0..2^20");
    if (batch > 0 && (!counts || !poses || !sums)) return refuse("sv_flow_pose_sums: counts, poses or sums is NULL");
    if (batch > 0 && capacity > 0 && !matches) return refuse("sv_flow_pose_sums: matches is NULL");
    if (any_misaligned(4, matches, counts)) return refuse("sv_flow_pose_sums: matches or counts is not 4-byte aligned");
    if (misaligned(poses, 8) || misaligned(sums, 8)) return refuse("sv_flow_pose_sums: poses or sums is not 8-byte aligned");
    size_t need;
    sv_flow_pose_sums_workspace(capacity, batch, &need);
    if (need > 0 && !workspace) return refuse("sv_flow_pose_sums: the workspace is NULL");
    if (misaligned(workspace, 8)) return refuse("sv_flow_pose_sums: the workspace is not 8-byte aligned");
    if (workspace_bytes < need) return refuse("sv_flow_pose_sums: the workspace is smaller than sv_flow_pose_sums_workspace asks for");
    if (batch == 0) return SV_OK;  // nothing to do

    sv::FlowSumsArgs a;
    memset(&a, 0, sizeof(a));
    a.matches = matches, a.counts = counts, a.poses = poses;
    a.cam = camera_of(spec);
    a.B = batch, a.cap = capacity, a.n_chunks = chunks_of(capacity);
    a.gate_q = gate_q, a.dgate_q = dgate_q;
    a.partials = static_cast<unsigned long long *>(workspace);
    a.sums = reinterpret_cast<long long *>(sums);
    if (sv::launch_flow_sums(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_flow_pose_sums: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
