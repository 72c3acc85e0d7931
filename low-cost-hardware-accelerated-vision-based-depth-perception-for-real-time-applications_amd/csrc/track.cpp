// Group (AB) of include/stereo_vision_hip.h: the boxes of two frames linked by their temporal matches, and each linked box's own motion
// (track_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything is enqueued, and a
// refused call leaves its text for sv_last_error(NULL).
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "stage_glue.h"
#include "track_kernels.h"

namespace {

using namespace sv::glue;

std::atomic<int> g_flags{0};  // sv_debug_object_links

// NULL for a spec the kernels can use, else what is wrong with it.
const char *check_spec(const char *prefix, const sv_track_spec *s) {
    if (!s) return prefixed(prefix, "spec is NULL");
    for (int k = 0; k < 9; k++)
        if (s->reserved[k] != 0) return prefixed(prefix, "a reserved word of the spec is not 0");
    if (const char *bad = check_camera_words(prefix, s)) return bad;
    if (s->width < 1 || s->width > 8192 || s->height < 1 || s->height > 8192) return prefixed(prefix, "width or height outside 1..8192");
    if (s->max_boxes < 0 || s->max_boxes > sv::TRACK_BOXES_MAX) return prefixed(prefix, "max_boxes outside 0..64");
    if (s->band_q < 0 || s->band_q > sv::TRACK_BAND_MAX) return prefixed(prefix, "band_q outside 0..2^20");
    if (s->min_votes < 1) return prefixed(prefix, "min_votes < 1");
    if (s->share < 0 || s->share > sv::TRACK_SHARE_MAX) return prefixed(prefix, "share outside 0..256");
    if (s->gate_m < 0 || s->gate_m > sv::TRACK_GATE_MAX) return prefixed(prefix, "gate_m outside 0..2^20");
    return nullptr;
}

const char *check_sizes(const char *prefix, int capacity, int batch) {
    if (capacity < 0 || capacity > sv::FLOW_CAPACITY_MAX) return prefixed(prefix, "capacity outside 0..65536");
    if (batch < 0 || batch > 65535) return prefixed(prefix, "batch outside 0..65535");
    return nullptr;
}

}  // namespace

extern "C" {

int sv_object_links_workspace(int capacity, int batch, size_t *bytes) {
    if (!bytes) return refuse("sv_object_links_workspace: bytes is NULL");
    if (const char *bad = check_sizes("sv_object_links_workspace", capacity, batch)) return refuse(bad);
    *bytes = (size_t)batch * (size_t)capacity * 2 * sizeof(unsigned long long);
    return SV_OK;
}

int sv_object_links_device(const int32_t *matches, const int32_t *counts, const double *poses, int batch, int capacity, const int32_t *boxes0, const int32_t *n0,
                           const int32_t *q0, const int32_t *boxes1, const int32_t *n1, const int32_t *q1, const int32_t *centre, const sv_track_spec *spec,
                           int32_t *votes, int32_t *link, int64_t *sums, void *workspace, size_t workspace_bytes, void *stream) {
    if (const char *bad = check_sizes("sv_object_links", capacity, batch)) return refuse(bad);
    if (const char *bad = check_spec("sv_object_links", spec)) return refuse(bad);
    const size_t M = (size_t)spec->max_boxes, rows = (size_t)batch * M;
    if (batch > 0 && (!counts || !poses)) return refuse("sv_object_links: counts or poses is NULL");
    if (batch > 0 && capacity > 0 && !matches) return refuse("sv_object_links: matches is NULL");
    if (rows > 0 && (!boxes0 || !q0 || !boxes1 || !q1)) return refuse("sv_object_links: boxes0, q0, boxes1 or q1 is NULL");
    if (rows > 0 && (!votes || !link || !sums)) return refuse("sv_object_links: votes, link or sums is NULL");
    if (any_misaligned(4, matches, counts, boxes0, n0, q0) || any_misaligned(4, boxes1, n1, q1, centre) || any_misaligned(4, votes, link))
        return refuse("sv_object_links: matches, counts, a box array, centre, votes or link is not 4-byte aligned");
    if (misaligned(poses, 8) || misaligned(sums, 8)) return refuse("sv_object_links: poses or sums is not 8-byte aligned");
    size_t need;
    sv_object_links_workspace(capacity, batch, &need);
    if (need > 0 && rows > 0 && !workspace) return refuse("sv_object_links: the workspace is NULL");
    if (misaligned(workspace, 8)) return refuse("sv_object_links: the workspace is not 8-byte aligned");
    if (workspace_bytes < need) return refuse("sv_object_links: the workspace is smaller than sv_object_links_workspace asks for");
    const size_t nb = (size_t)batch * 4;
    const Span spans[] = {{matches, (size_t)batch * capacity * 24}, {counts, nb}, {poses, (size_t)batch * 96}, {boxes0, rows * 16}, {n0, nb}, {q0, rows * 4},
                          {boxes1, rows * 16}, {n1, nb}, {q1, rows * 4}, {centre, rows * 12}, {workspace, rows ? need : 0}, {votes, rows * (M + 1) * 4},
                          {link, rows * 16}, {sums, rows * sv::TRACK_SUM_WORDS * 8}};
    if (outputs_overlap(spans, 14, 10)) return refuse("sv_object_links: an output or the workspace shares bytes with an input or another output");
    if (rows == 0) return SV_OK;  // nothing to write

    sv::TrackArgs a;
    memset(&a, 0, sizeof(a));
    a.matches = matches, a.counts = counts, a.poses = poses;
    a.cam = sv::FlowCamera{spec->f, spec->cx, spec->cy, spec->b16, spec->fb, spec->fb16};
    a.boxes0 = boxes0, a.boxes1 = boxes1, a.n0 = n0, a.n1 = n1, a.q0 = q0, a.q1 = q1, a.centre = centre;
    a.B = batch, a.cap = capacity, a.M = spec->max_boxes, a.W = spec->width, a.H = spec->height;
    a.n_chunks = (capacity + sv::TRACK_THREADS - 1) / sv::TRACK_THREADS;
    a.min_votes = spec->min_votes, a.share = spec->share, a.flags = g_flags.load();
    a.band_q = spec->band_q, a.gate_m = spec->gate_m;
    a.words = static_cast<unsigned long long *>(workspace);
    a.votes = votes, a.link = link, a.sums = reinterpret_cast<unsigned long long *>(sums);
    if (sv::launch_object_links(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_object_links: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_debug_object_links(int flags) {
    if (flags & ~(int)sv::TRACK_STOP_MASK) return refuse("sv_debug_object_links: flags outside 0..3");
    g_flags.store(flags);
    return SV_OK;
}

} /* extern "C" */
