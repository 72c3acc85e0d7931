// The pose graph of confirmed loops: include/stereo_vision_hip.h (AE), restated in stereo_vision/sv.py (pose_graph_linearize,
// pose_graph_pcg, pose_graph_sum).  Every double is formed one operation at a time in the order the definition states - the build has
// -ffp-contract=off, so a * b + c is two roundings -, there is no trigonometry and no square root (the factor is L D L^T), and a double
// division is correctly rounded: the results equal the numpy form bit for bit.
//
//   linearise  lin_edges: a lane per edge - M = P_j^-1 o P_i, W r, chi2.  lin_poses: a lane per pose walks its incidence list in
//              ascending order for b and the 6 x 6 diagonal block, adds lam and factors the block in registers.
//   PCG        three kernels per iteration t, all of 256 threads:
//                edges   a lane per edge: p_i and p_j are formed on the fly as z + beta p_before (z in iteration 0), g = W (p_j - Ad_M p_i)
//                poses   a lane per pose: the verdict rr <= tol^2 rr0 first; then p = z + beta p_before is written, q = H p is gathered over
//                        the incidence list, and the workgroup's partial of <p, q> leaves it
//                update  a lane per pose: alpha = rz / <p, q>; x += alpha p; r -= alpha q; z = F^-1 r; the partials of <r, r> and <r, z>
//              A dot product is never finished by an atomic or a kernel of its own: the workgroup of a pose kernel is a chunk of
//              pose_graph_sum, its halving tree gives the chunk's partial, and every workgroup of the next kernel reduces the partials
//              (at most 4096) by the same rule, so all hold the same bits.  The partials of <r, r> and <r, z> lie in two buffers by the
//              parity of t: the update kernel reads one pair and writes the other, and beta = rz / rz_before reads both.
//   state      iteration, done, rr, rr0 in device memory.  Every kernel reads a done word first and returns when it is set; the word a
//              kernel reads is written by another kernel (`done` by poses, the start and the finish; `done_seen` by update), never by
//              one of its own workgroups.  The host enqueues a fixed number of iterations and never waits.
//
// Nothing is allocated, no atomic is used, and every loop ends by the data alone: the walk of an incidence list is bounded by
// row_start, a reduction by the count of chunks.  Every index read from memory - an edge's poses, an entry's edge - is compared with
// its bound before it is used; what fails counts as absent.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pose_graph_kernels.h"

namespace sv {

namespace {

__device__ __forceinline__ void pg_mv(const double *R, const double *x, double *y) {  // y = R x
#pragma unroll
    for (int a = 0; a < 3; a++) y[a] = (R[3 * a] * x[0] + R[3 * a + 1] * x[1]) + R[3 * a + 2] * x[2];
}

__device__ __forceinline__ void pg_mtv(const double *R, const double *x, double *y) {  // y = R^T x
#pragma unroll
    for (int a = 0; a < 3; a++) y[a] = (R[a] * x[0] + R[3 + a] * x[1]) + R[6 + a] * x[2];
}

__device__ __forceinline__ void pg_cross(const double *t, const double *u, double *c) {
    c[0] = t[1] * u[2] - t[2] * u[1];
    c[1] = t[2] * u[0] - t[0] * u[2];
    c[2] = t[0] * u[1] - t[1] * u[0];
}

// y = Ad_M x, x = (om, v): (R om, t x (R om) + R v)
__device__ __forceinline__ void pg_ad(const double *M, const double *x, double *y) {
    double v[3], c[3];
    pg_mv(M, x, y);
    pg_mv(M, x + 3, v);
    pg_cross(M + 9, y, c);
#pragma unroll
    for (int a = 0; a < 3; a++) y[3 + a] = c[a] + v[a];
}

// y = Ad_M^T g, g = (g_rot, g_trans): (R^T (g_rot - t x g_trans), R^T g_trans)
__device__ __forceinline__ void pg_adt(const double *M, const double *g, double *y) {
    double c[3], d[3];
    pg_cross(M + 9, g + 3, c);
#pragma unroll
    for (int a = 0; a < 3; a++) d[a] = g[a] - c[a];
    pg_mtv(M, d, y);
    pg_mtv(M, g + 3, y + 3);
}

__device__ __forceinline__ double pg_dot6(const double *a, const double *b) {
    double s = a[0] * b[0];
#pragma unroll
    for (int c = 1; c < 6; c++) s = s + a[c] * b[c];
    return s;
}

__device__ __forceinline__ constexpr int pg_at(int p, int q) { return p * (p + 1) / 2 + q; }

// z = (L D L^T)^-1 r of one pose
__device__ __forceinline__ void pg_precondition(const double *F, const double *r, double *z) {
    double y[6];
#pragma unroll
    for (int p = 0; p < 6; p++) {
        double s = r[p];
#pragma unroll
        for (int q = 0; q < p; q++) s = s - F[pg_at(p, q)] * y[q];
        y[p] = s;
    }
#pragma unroll
    for (int p = 0; p < 6; p++) y[p] = y[p] / F[pg_at(p, p)];
#pragma unroll
    for (int p = 5; p >= 0; p--) {
        double s = y[p];
#pragma unroll
        for (int q = p + 1; q < 6; q++) s = s - F[pg_at(q, p)] * z[q];
        z[p] = s;
    }
}

// The halving tree over the 64 lanes of a wavefront as a butterfly: lane k < h holds v[k] + v[k + h] after the step of h, as the tree
// asks; the lanes above hold the mirror image, and an addition commutes, so every lane ends with lane 0's bits.
__device__ __forceinline__ double pg_wave_tree(double v) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_xor(v, h);
    return v;
}

// The halving tree over the 256 values of a workgroup, one per thread -> the sum, in every thread.  Every thread of the workgroup
// must call it; s_tree is free again on return.
__device__ __forceinline__ double pg_block_tree(double v, double *s_tree) {
    const int tid = threadIdx.x;
    s_tree[tid] = v;
    __syncthreads();
    if (tid < 128) s_tree[tid] = s_tree[tid] + s_tree[tid + 128];  // reads 128 .. 255, writes 0 .. 127
    __syncthreads();
    if (tid < 64) {  // the first wavefront, whole
        v = pg_wave_tree(s_tree[tid] + s_tree[tid + 64]);
        if (tid == 0) s_tree[256] = v;
    }
    __syncthreads();
    v = s_tree[256];
    __syncthreads();
    return v;
}

// pose_graph_sum over the `chunks` partials of a dot product, whose first level the writers made: none left to make for one partial,
// one for at most 256, two for at most 4096 (2^20 poses).  The same in every thread of every workgroup.
__device__ __forceinline__ double pg_finish(const double *partials, int chunks, double *s_tree) {
    const int tid = threadIdx.x;
    if (chunks == 1) return partials[0];
    if (chunks <= PG_THREADS) return pg_block_tree(tid < chunks ? partials[tid] : 0.0, s_tree);
    const int upper = (chunks + PG_THREADS - 1) / PG_THREADS;  // <= 16
    double mine = 0.0;
    for (int c = 0; c < upper; c++) {
        const int at = c * PG_THREADS + tid;
        const double s = pg_block_tree(at < chunks ? partials[at] : 0.0, s_tree);
        if (tid == c) mine = s;
    }
    return pg_block_tree(mine, s_tree);
}

// The entries of pose k in inc, [at, end): row_start's, kept inside the 2 n_edges words inc holds whatever row_start says.
__device__ __forceinline__ void pg_entries(const int32_t *row_start, int k, int n_edges, int &at, int &end) {
    const int top = 2 * n_edges;  // <= 2^23
    at = row_start[k], end = row_start[k + 1];
    at = at < 0 ? 0 : at;
    end = end > top ? top : end;
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_lin_edges(PoseGraphLinArgs a) {
    const int e = blockIdx.x * PG_THREADS + threadIdx.x;
    if (e >= a.n_edges) return;
    const unsigned i = (unsigned)a.ei[e], j = (unsigned)a.ej[e];
    double M[12], Wr[6], chi2 = 0.0;
    if (i >= (unsigned)a.n_poses || j >= (unsigned)a.n_poses) {  // refused by every caller of this library: kept from the memory
#pragma unroll
        for (int c = 0; c < 12; c++) M[c] = 0.0;
#pragma unroll
        for (int c = 0; c < 6; c++) Wr[c] = 0.0;
    } else {
        double Pi[12], Pj[12], Z[12], d[3], RQ[9], tQ[3], u[3], tD[3];
#pragma unroll
        for (int c = 0; c < 12; c++) Pi[c] = a.poses[12 * (size_t)i + c], Pj[c] = a.poses[12 * (size_t)j + c], Z[c] = a.Z[12 * (size_t)e + c];
        const double wr = a.w[2 * (size_t)e], wt = a.w[2 * (size_t)e + 1];
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) M[3 * r + c] = (Pj[r] * Pi[c] + Pj[3 + r] * Pi[3 + c]) + Pj[6 + r] * Pi[6 + c];
#pragma unroll
        for (int c = 0; c < 3; c++) d[c] = Pi[9 + c] - Pj[9 + c];
        pg_mtv(Pj, d, M + 9);
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) RQ[3 * r + c] = (M[3 * r] * Z[c] + M[3 * r + 1] * Z[3 + c]) + M[3 * r + 2] * Z[6 + c];
        pg_mv(M, Z + 9, u);
#pragma unroll
        for (int c = 0; c < 3; c++) tQ[c] = u[c] + M[9 + c];
        const double rot[3] = {0.5 * (RQ[5] - RQ[7]), 0.5 * (RQ[6] - RQ[2]), 0.5 * (RQ[1] - RQ[3])};
        pg_mtv(RQ, tQ, tD);
#pragma unroll
        for (int c = 0; c < 3; c++) tD[c] = -tD[c];
#pragma unroll
        for (int c = 0; c < 3; c++) Wr[c] = wr * rot[c], Wr[3 + c] = wt * tD[c];
        chi2 = wr * ((rot[0] * rot[0] + rot[1] * rot[1]) + rot[2] * rot[2]) + wt * ((tD[0] * tD[0] + tD[1] * tD[1]) + tD[2] * tD[2]);
    }
#pragma unroll
    for (int c = 0; c < 12; c++) a.M[12 * (size_t)e + c] = M[c];
#pragma unroll
    for (int c = 0; c < 6; c++) a.Wr[6 * (size_t)e + c] = Wr[c];
    a.chi2[e] = chi2;
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_lin_poses(PoseGraphLinArgs a) {
    const int k = blockIdx.x * PG_THREADS + threadIdx.x;
    if (k >= a.n_poses) return;
    double acc[6], B[PG_BLOCK_WORDS];
#pragma unroll
    for (int c = 0; c < 6; c++) acc[c] = 0.0;
#pragma unroll
    for (int n = 0; n < PG_BLOCK_WORDS; n++) B[n] = 0.0;
    int at, end;
    pg_entries(a.row_start, k, a.n_edges, at, end);
    for (; at < end; at++) {
        const int code = a.inc[at];
        const unsigned e = (unsigned)code >> 1;
        if (code < 0 || e >= (unsigned)a.n_edges) continue;
        double Wr[6];
#pragma unroll
        for (int c = 0; c < 6; c++) Wr[c] = a.Wr[6 * (size_t)e + c];
        const double wr = a.w[2 * (size_t)e], wt = a.w[2 * (size_t)e + 1];
        if (code & 1) {  // the pose is the edge's i
            double M[12], up[6], A[6][6];
#pragma unroll
            for (int c = 0; c < 12; c++) M[c] = a.M[12 * (size_t)e + c];
            pg_adt(M, Wr, up);
#pragma unroll
            for (int c = 0; c < 6; c++) acc[c] = acc[c] + up[c];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double col[3] = {M[c], M[3 + c], M[6 + c]};
                double T[3];
                pg_cross(M + 9, col, T);
#pragma unroll
                for (int r = 0; r < 3; r++) A[r][c] = M[3 * r + c], A[r][3 + c] = 0.0, A[3 + r][3 + c] = M[3 * r + c], A[3 + r][c] = T[r];
            }
#pragma unroll
            for (int p = 0; p < 6; p++)
#pragma unroll
                for (int q = 0; q <= p; q++) {
                    double s = (A[0][p] * wr) * A[0][q];
#pragma unroll
                    for (int m = 1; m < 6; m++) s = s + (A[m][p] * (m < 3 ? wr : wt)) * A[m][q];
                    B[pg_at(p, q)] = B[pg_at(p, q)] + s;
                }
        } else {
#pragma unroll
            for (int c = 0; c < 6; c++) acc[c] = acc[c] - Wr[c];
#pragma unroll
            for (int p = 0; p < 6; p++) B[pg_at(p, p)] = B[pg_at(p, p)] + (p < 3 ? wr : wt);
        }
    }
#pragma unroll
    for (int p = 0; p < 6; p++) B[pg_at(p, p)] = B[pg_at(p, p)] + a.lam;
#pragma unroll
    for (int p = 0; p < 6; p++) {
        double s = B[pg_at(p, p)];
#pragma unroll
        for (int q = 0; q < p; q++) s = s - (B[pg_at(p, q)] * B[pg_at(q, q)]) * B[pg_at(p, q)];
        B[pg_at(p, p)] = s;
#pragma unroll
        for (int r = p + 1; r < 6; r++) {
            double t = B[pg_at(r, p)];
#pragma unroll
            for (int q = 0; q < p; q++) t = t - (B[pg_at(r, q)] * B[pg_at(q, q)]) * B[pg_at(p, q)];
            B[pg_at(r, p)] = t / s;
        }
    }
    const bool fixed = a.fixed[k] != 0;
#pragma unroll
    for (int c = 0; c < 6; c++) a.b[6 * (size_t)k + c] = fixed ? 0.0 : acc[c];
#pragma unroll
    for (int n = 0; n < PG_BLOCK_WORDS; n++) a.factor[PG_BLOCK_WORDS * (size_t)k + n] = B[n];
}

// x = 0, r = b, z = F^-1 r, and the chunk's partials of <r, r> and <r, z> for iteration 0.
__global__ __launch_bounds__(PG_THREADS) void k_pg_start(PoseGraphPcgArgs a) {
    __shared__ double s_tree[PG_THREADS + 1];
    const int k = blockIdx.x * PG_THREADS + threadIdx.x;
    double rr = 0.0, rz = 0.0;
    if (k < a.n_poses) {
        double r[6], z[6], F[PG_BLOCK_WORDS];
#pragma unroll
        for (int c = 0; c < 6; c++) r[c] = a.b[6 * (size_t)k + c];
#pragma unroll
        for (int n = 0; n < PG_BLOCK_WORDS; n++) F[n] = a.factor[PG_BLOCK_WORDS * (size_t)k + n];
        pg_precondition(F, r, z);
#pragma unroll
        for (int c = 0; c < 6; c++) a.x[6 * (size_t)k + c] = 0.0, a.r[6 * (size_t)k + c] = r[c], a.z[6 * (size_t)k + c] = z[c];
        rr = pg_dot6(r, r), rz = pg_dot6(r, z);
    }
    rr = pg_block_tree(rr, s_tree);
    rz = pg_block_tree(rz, s_tree);
    if (threadIdx.x == 0) a.prr[0][blockIdx.x] = rr, a.prz[0][blockIdx.x] = rz;
}

// One workgroup: the state words of a solve that starts.
__global__ __launch_bounds__(PG_THREADS) void k_pg_start_state(PoseGraphPcgArgs a) {
    __shared__ double s_tree[PG_THREADS + 1];
    const double rr0 = pg_finish(a.prr[0], a.chunks, s_tree);
    if (threadIdx.x != 0) return;
    const int done = rr0 <= a.tol2 * rr0 ? 1 : 0;
    PoseGraphState s = {};
    s.iteration = 0, s.done = done, s.rr = rr0, s.rr0 = rr0, s.done_seen = done;
    *a.state = s;
}

// beta of iteration t >= 1: rz over rz_before, from the two pairs of partials.  Every thread of the workgroup must call it.
__device__ __forceinline__ double pg_beta(const PoseGraphPcgArgs &a, int t, double *s_tree) {
    const double rz = pg_finish(a.prz[t & 1], a.chunks, s_tree);
    return rz / pg_finish(a.prz[(t & 1) ^ 1], a.chunks, s_tree);
}

__device__ __forceinline__ void pg_direction(const PoseGraphPcgArgs &a, int t, double beta, unsigned k, double *p) {
#pragma unroll
    for (int c = 0; c < 6; c++) p[c] = a.z[6 * (size_t)k + c];
    if (t > 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) p[c] = p[c] + beta * a.p[6 * (size_t)k + c];
    }
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_edges(PoseGraphPcgArgs a, int t) {
    __shared__ double s_tree[PG_THREADS + 1];
    if (a.state->done) return;
    const double beta = t > 0 ? pg_beta(a, t, s_tree) : 0.0;
    const int e = blockIdx.x * PG_THREADS + threadIdx.x;
    if (e >= a.n_edges) return;  // behind the last barrier
    const unsigned i = (unsigned)a.ei[e], j = (unsigned)a.ej[e];
    double g[6];
    if (i >= (unsigned)a.n_poses || j >= (unsigned)a.n_poses) {
#pragma unroll
        for (int c = 0; c < 6; c++) g[c] = 0.0;
    } else {
        double M[12], pi[6], pj[6], ad[6];
#pragma unroll
        for (int c = 0; c < 12; c++) M[c] = a.M[12 * (size_t)e + c];
        pg_direction(a, t, beta, i, pi);
        pg_direction(a, t, beta, j, pj);
        pg_ad(M, pi, ad);
        const double wr = a.w[2 * (size_t)e], wt = a.w[2 * (size_t)e + 1];
#pragma unroll
        for (int c = 0; c < 6; c++) g[c] = (c < 3 ? wr : wt) * (pj[c] - ad[c]);
    }
#pragma unroll
    for (int c = 0; c < 6; c++) a.g[6 * (size_t)e + c] = g[c];
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_poses(PoseGraphPcgArgs a, int t) {
    __shared__ double s_tree[PG_THREADS + 1];
    if (a.state->done_seen) return;
    const double rr = pg_finish(a.prr[t & 1], a.chunks, s_tree);
    if (rr <= a.tol2 * a.state->rr0) {  // the same verdict in every workgroup
        if (blockIdx.x == 0 && threadIdx.x == 0) a.state->done = 1, a.state->rr = rr;
        return;
    }
    const double beta = t > 0 ? pg_beta(a, t, s_tree) : 0.0;
    const int k = blockIdx.x * PG_THREADS + threadIdx.x;
    double pq = 0.0;
    if (k < a.n_poses) {
        double p[6], q[6];
        pg_direction(a, t, beta, (unsigned)k, p);
#pragma unroll
        for (int c = 0; c < 6; c++) q[c] = 0.0;
        int at, end;
        pg_entries(a.row_start, k, a.n_edges, at, end);
        for (; at < end; at++) {
            const int code = a.inc[at];
            const unsigned e = (unsigned)code >> 1;
            if (code < 0 || e >= (unsigned)a.n_edges) continue;
            double g[6];
#pragma unroll
            for (int c = 0; c < 6; c++) g[c] = a.g[6 * (size_t)e + c];
            if (code & 1) {
                double M[12], down[6];
#pragma unroll
                for (int c = 0; c < 12; c++) M[c] = a.M[12 * (size_t)e + c];
                pg_adt(M, g, down);
#pragma unroll
                for (int c = 0; c < 6; c++) q[c] = q[c] - down[c];
            } else {
#pragma unroll
                for (int c = 0; c < 6; c++) q[c] = q[c] + g[c];
            }
        }
        const bool fixed = a.fixed[k] != 0;
#pragma unroll
        for (int c = 0; c < 6; c++) {
            q[c] = fixed ? 0.0 : q[c] + a.lam * p[c];
            a.p[6 * (size_t)k + c] = p[c], a.q[6 * (size_t)k + c] = q[c];
        }
        pq = pg_dot6(p, q);
    }
    pq = pg_block_tree(pq, s_tree);
    if (threadIdx.x == 0) {
        a.ppq[blockIdx.x] = pq;
        if (blockIdx.x == 0) a.state->iteration = t + 1, a.state->rr = rr;
    }
}

__global__ __launch_bounds__(PG_THREADS) void k_pg_update(PoseGraphPcgArgs a, int t) {
    __shared__ double s_tree[PG_THREADS + 1];
    if (a.state->done) {
        if (blockIdx.x == 0 && threadIdx.x == 0) a.state->done_seen = 1;
        return;
    }
    const double rz_now = pg_finish(a.prz[t & 1], a.chunks, s_tree);
    const double alpha = rz_now / pg_finish(a.ppq, a.chunks, s_tree);
    const int k = blockIdx.x * PG_THREADS + threadIdx.x;
    double rr = 0.0, rz = 0.0;
    if (k < a.n_poses) {
        double r[6], z[6], F[PG_BLOCK_WORDS];
#pragma unroll
        for (int c = 0; c < 6; c++) {
            const size_t at = 6 * (size_t)k + c;
            a.x[at] = a.x[at] + alpha * a.p[at];
            r[c] = a.r[at] - alpha * a.q[at];
            a.r[at] = r[c];
        }
#pragma unroll
        for (int n = 0; n < PG_BLOCK_WORDS; n++) F[n] = a.factor[PG_BLOCK_WORDS * (size_t)k + n];
        pg_precondition(F, r, z);
#pragma unroll
        for (int c = 0; c < 6; c++) a.z[6 * (size_t)k + c] = z[c];
        rr = pg_dot6(r, r), rz = pg_dot6(r, z);
    }
    rr = pg_block_tree(rr, s_tree);
    rz = pg_block_tree(rz, s_tree);
    const int next = (t & 1) ^ 1;
    if (threadIdx.x == 0) a.prr[next][blockIdx.x] = rr, a.prz[next][blockIdx.x] = rz;
}

// One workgroup behind the last iteration of a call: rr of the residual as it stands, and the verdict on it.
__global__ __launch_bounds__(PG_THREADS) void k_pg_finish(PoseGraphPcgArgs a, int t) {
    __shared__ double s_tree[PG_THREADS + 1];
    if (a.state->done) return;
    const double rr = pg_finish(a.prr[t & 1], a.chunks, s_tree);
    if (threadIdx.x != 0) return;
    a.state->rr = rr;
    if (rr <= a.tol2 * a.state->rr0) a.state->done = 1, a.state->done_seen = 1;
}

inline unsigned groups_of(int n) { return (unsigned)((n + PG_THREADS - 1) / PG_THREADS); }

}  // namespace

hipError_t launch_pose_graph_linearize(const PoseGraphLinArgs &a, hipStream_t st) {
    if (a.n_edges > 0) {
        hipLaunchKernelGGL(k_pg_lin_edges, dim3(groups_of(a.n_edges)), dim3(PG_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    hipLaunchKernelGGL(k_pg_lin_poses, dim3(groups_of(a.n_poses)), dim3(PG_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pose_graph_pcg(const PoseGraphPcgArgs &a, int iter0, int iters, hipStream_t st) {
    const dim3 poses(groups_of(a.n_poses)), edges(groups_of(a.n_edges)), threads(PG_THREADS);
    if (iter0 == 0) {
        hipLaunchKernelGGL(k_pg_start, poses, threads, 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
        hipLaunchKernelGGL(k_pg_start_state, dim3(1), threads, 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    for (int t = iter0; t < iter0 + iters; t++) {
        if (a.n_edges > 0) hipLaunchKernelGGL(k_pg_edges, edges, threads, 0, st, a, t);
        hipLaunchKernelGGL(k_pg_poses, poses, threads, 0, st, a, t);
        hipLaunchKernelGGL(k_pg_update, poses, threads, 0, st, a, t);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    hipLaunchKernelGGL(k_pg_finish, dim3(1), threads, 0, st, a, iter0 + iters);
    return hipGetLastError();
}

}  // namespace sv
