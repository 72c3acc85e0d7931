// Group (AE) of include/stereo_vision_hip.h: the pose graph of confirmed loops - one linearisation, and preconditioned conjugate
// gradients on it (pose_graph_kernels.hip).  Everything here is argument checking and launch set-up; every check runs before anything
// is enqueued, a refused call leaves its text for sv_last_error(NULL), no entry waits for the GPU, and none reads the data it is given.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/stereo_vision_hip.h"
#include "pose_graph_kernels.h"
#include "stage_glue.h"

namespace {

using namespace sv::glue;

constexpr int MAX_POSES = 1 << 20;
constexpr int MAX_EDGES = 1 << 22;
constexpr int MAX_ITERS = 1024;        // iterations a call may enqueue
constexpr int MAX_ITER0 = 1 << 30;

const char *check_sizes(const char *prefix, int n_poses, int n_edges) {
    if (n_poses < 1 || n_poses > MAX_POSES) return prefixed(prefix, "n_poses outside 1 .. 2^20");
    if (n_edges < 0 || n_edges > MAX_EDGES) return prefixed(prefix, "n_edges outside 0 .. 2^22");
    return nullptr;
}

const char *check_spec(const char *prefix, const sv_pose_graph_spec *s) {
    if (!s) return prefixed(prefix, "spec is NULL");
    for (int k = 0; k < 12; k++)
        if (s->reserved[k] != 0) return prefixed(prefix, "a reserved word of the spec is not 0");
    if (!(s->lam > 0.0) || !isfinite(s->lam)) return prefixed(prefix, "lam is not a finite number > 0");
    if (!(s->tol >= 0.0) || !isfinite(s->tol)) return prefixed(prefix, "tol is negative or not finite");
    return nullptr;
}

// The workspace: the state words, then r, z, p, q, then g, then the five rows of partials.
struct Layout {
    size_t vec, g, part, total;
    int chunks;
};

Layout layout_of(int n_poses, int n_edges) {
    Layout l;
    l.chunks = (n_poses + sv::PG_THREADS - 1) / sv::PG_THREADS;
    l.vec = align16((size_t)n_poses * 6 * sizeof(double));
    l.g = align16((size_t)n_edges * 6 * sizeof(double));
    l.part = align16((size_t)l.chunks * sizeof(double));
    l.total = sv::PG_STATE_BYTES + 4 * l.vec + l.g + 5 * l.part;
    return l;
}

}  // namespace

extern "C" {

int sv_pose_graph_workspace(int n_poses, int n_edges, size_t *bytes) {
    if (!bytes) return refuse("sv_pose_graph_workspace: bytes is NULL");
    if (const char *bad = check_sizes("sv_pose_graph_workspace", n_poses, n_edges)) return refuse(bad);
    *bytes = layout_of(n_poses, n_edges).total;
    return SV_OK;
}

int sv_pose_graph_linearize_device(const double *poses, const uint8_t *fixed, int n_poses, const int32_t *ei, const int32_t *ej, const double *Z, const double *w,
                                   int n_edges, const int32_t *row_start, const int32_t *inc, const sv_pose_graph_spec *spec, double *M, double *Wr, double *chi2,
                                   double *b, double *factor, void *stream) {
    if (const char *bad = check_sizes("sv_pose_graph_linearize", n_poses, n_edges)) return refuse(bad);
    if (const char *bad = check_spec("sv_pose_graph_linearize", spec)) return refuse(bad);
    if (!poses || !fixed || !row_start || !b || !factor) return refuse("sv_pose_graph_linearize: poses, fixed, row_start, b or factor is NULL");
    if (n_edges > 0 && (!ei || !ej || !Z || !w || !inc || !M || !Wr || !chi2)) return refuse("sv_pose_graph_linearize: an array of the edges is NULL");
    if (any_misaligned(8, poses, Z, w, M, Wr, chi2, b, factor)) return refuse("sv_pose_graph_linearize: an array of doubles is not 8-byte aligned");
    if (any_misaligned(4, ei, ej, row_start, inc)) return refuse("sv_pose_graph_linearize: an array of int32 is not 4-byte aligned");
    const size_t N = (size_t)n_poses, E = (size_t)n_edges;
    const Span spans[13] = {{poses, N * 96}, {fixed, N},     {ei, E * 4},  {ej, E * 4}, {Z, E * 96}, {w, E * 16},     {row_start, (N + 1) * 4},
                            {inc, E * 8},    {M, E * 96},    {Wr, E * 48}, {chi2, E * 8}, {b, N * 48}, {factor, N * 168}};
    if (outputs_overlap(spans, 13, 8)) return refuse("sv_pose_graph_linearize: an output overlaps an input or another output");

    sv::PoseGraphLinArgs a;
    memset(&a, 0, sizeof(a));
    a.poses = poses, a.fixed = fixed, a.ei = ei, a.ej = ej, a.Z = Z, a.w = w, a.row_start = row_start, a.inc = inc;
    a.M = M, a.Wr = Wr, a.chi2 = chi2, a.b = b, a.factor = factor, a.lam = spec->lam, a.n_poses = n_poses, a.n_edges = n_edges;
    if (sv::launch_pose_graph_linearize(a, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_pose_graph_linearize: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

int sv_pose_graph_pcg_device(const uint8_t *fixed, int n_poses, const int32_t *ei, const int32_t *ej, const double *w, int n_edges, const int32_t *row_start,
                             const int32_t *inc, const double *M, const double *b, const double *factor, const sv_pose_graph_spec *spec, int iter0, int iters,
                             double *x, void *workspace, size_t workspace_bytes, void *stream) {
    if (const char *bad = check_sizes("sv_pose_graph_pcg", n_poses, n_edges)) return refuse(bad);
    if (const char *bad = check_spec("sv_pose_graph_pcg", spec)) return refuse(bad);
    if (iter0 < 0 || iter0 > MAX_ITER0) return refuse("sv_pose_graph_pcg: iter0 outside 0 .. 2^30");
    if (iters < 0 || iters > MAX_ITERS) return refuse("sv_pose_graph_pcg: iters outside 0 .. 1024");
    if (!fixed || !row_start || !b || !factor || !x || !workspace) return refuse("sv_pose_graph_pcg: fixed, row_start, b, factor, x or the workspace is NULL");
    if (n_edges > 0 && (!ei || !ej || !w || !inc || !M)) return refuse("sv_pose_graph_pcg: an array of the edges is NULL");
    if (any_misaligned(8, w, M, b, factor, x)) return refuse("sv_pose_graph_pcg: an array of doubles is not 8-byte aligned");
    if (any_misaligned(4, ei, ej, row_start, inc)) return refuse("sv_pose_graph_pcg: an array of int32 is not 4-byte aligned");
    if (misaligned(workspace, 16)) return refuse("sv_pose_graph_pcg: the workspace is not 16-byte aligned");
    const Layout l = layout_of(n_poses, n_edges);
    if (workspace_bytes < l.total) return refuse("sv_pose_graph_pcg: the workspace is smaller than sv_pose_graph_workspace asks for");
    const size_t N = (size_t)n_poses, E = (size_t)n_edges;
    const Span spans[11] = {{fixed, N}, {ei, E * 4}, {ej, E * 4}, {w, E * 16}, {row_start, (N + 1) * 4}, {inc, E * 8}, {M, E * 96}, {b, N * 48},
                            {factor, N * 168}, {x, N * 48}, {workspace, l.total}};
    if (outputs_overlap(spans, 11, 9)) return refuse("sv_pose_graph_pcg: x and the workspace overlap one another or an input");

    sv::PoseGraphPcgArgs a;
    memset(&a, 0, sizeof(a));
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    a.fixed = fixed, a.ei = ei, a.ej = ej, a.w = w, a.row_start = row_start, a.inc = inc, a.M = M, a.b = b, a.factor = factor;
    a.lam = spec->lam, a.tol2 = spec->tol * spec->tol, a.x = x;
    a.state = reinterpret_cast<sv::PoseGraphState *>(ws);
    ws += sv::PG_STATE_BYTES;
    double **vecs[4] = {&a.r, &a.z, &a.p, &a.q};
    for (double **v : vecs) *v = reinterpret_cast<double *>(ws), ws += l.vec;
    a.g = reinterpret_cast<double *>(ws), ws += l.g;
    double **parts[5] = {&a.prr[0], &a.prr[1], &a.prz[0], &a.prz[1], &a.ppq};
    for (double **v : parts) *v = reinterpret_cast<double *>(ws), ws += l.part;
    a.n_poses = n_poses, a.n_edges = n_edges, a.chunks = l.chunks;
    if (sv::launch_pose_graph_pcg(a, iter0, iters, static_cast<hipStream_t>(stream)) != hipSuccess) {
        sv_internal_set_error("sv_pose_graph_pcg: a kernel launch failed");
        return SV_ERR_HIP;
    }
    return SV_OK;
}

} /* extern "C" */
