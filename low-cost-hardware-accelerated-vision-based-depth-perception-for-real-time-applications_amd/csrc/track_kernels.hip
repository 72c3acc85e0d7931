// The boxes of frame k - 1 linked to those of frame k by the temporal matches that lie in both, and each linked box's matches reduced to the
// box's own motion - include/stereo_vision_hip.h (AB), restated in stereo_vision/sv.py (object_links).  Doubles in the definition's order in
// front of the rounding (flow_point.h: the functions of group (Z); the build contracts nothing), integers behind it.  Four kernels:
//
//   clear   a lane per word of votes and sums.  Nothing is assumed of what the outputs or the workspace held.
//   votes   grid (chunk of 256 matches, frame), a lane per match.  The frame's 2 x 64 boxes, clamped, and their 4 q are staged in LDS once
//           per workgroup; a lane builds its two membership words in two uniform loops over the boxes and writes them to the workspace.
//           The votes are counted a wavefront at a time - per previous box that some lane is a member of, the union of those lanes' current
//           words, a ballot per set pair - and added into a table of 64 x 65 int32 in LDS by one lane; the workgroup flushes its non-zero
//           entries by integer atomicAdd.
//   link    a wavefront per frame: the frame's votes staged in LDS by coalesced loads (rows of M + 1 words: an odd pitch for M = 64, a lane
//           per row reads without bank conflicts), then a lane per previous box: the arg-max over j, the contest over i by shuffles.  No
//           atomic.
//   sums    grid as votes.  A lane reads its two words and the links (LDS) and, if it feeds a box, makes the doubles and adds its fifteen
//           words into a table [64][16] of 64-bit words in LDS, flushed by 64-bit integer atomicAdd.  On the KITTI frames a few hundred
//           matches of a frame feed a box, and the adds of a lane cost less than combining the wavefront by shuffles first (13 sums of
//           64-bit words, 12 shuffles each, per box the wavefront feeds; measured), so the lanes add for themselves.
//
// Integer atomics only: the bits do not depend on the schedule.
// bounds    a match is read for i < rows <= cap, its words are written for i < cap; bit k of a word is set only for k < n <= M <= 64, so a
//           vote lands in row k < M and column j < M or M, and a sum in row k < M; link[k] is a current box < M or -1.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "flow_point.h"
#include "track_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

typedef unsigned long long u64;

constexpr double TRACK_PIXEL_MAX = 1073741824.0;  // (Z2)'s |pu|, |pv|, |pd| of a match that is inside

__device__ __forceinline__ int track_clamp(long long a, int size) { return (int)(a < 0 ? 0 : a > size - 1 ? size - 1 : a); }

// a value that every lane holds alike, as two scalars: the loops over its bits are then the wavefront's, not a lane's
__device__ __forceinline__ u64 track_uniform(u64 v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 wave_or(u64 v) {
    return track_uniform(wave_reduce(v, [](u64 a, u64 o) { return a | o; }));
}

// clamp(floor(v + 0.5), +-lim) of a double that is not NaN
__device__ __forceinline__ long long track_q(double v, double lim) {
    const double r = floor(v + 0.5);
    return (long long)(r < -lim ? -lim : r > lim ? lim : r);
}
__device__ __forceinline__ long long track_clip(long long v, long long lim) { return v < -lim ? -lim : v > lim ? lim : v; }

__global__ __launch_bounds__(TRACK_THREADS) void k_track_clear(TrackArgs a) {
    const int b = (int)blockIdx.y, k = (int)(blockIdx.x * TRACK_THREADS + threadIdx.x);
    if (k < a.M * (a.M + 1)) a.votes[(size_t)b * a.M * (a.M + 1) + k] = 0;
    if (k < a.M * TRACK_SUM_WORDS) a.sums[(size_t)b * a.M * TRACK_SUM_WORDS + k] = 0ull;
}

__global__ __launch_bounds__(TRACK_THREADS) void k_track_votes(TrackArgs a) {
    __shared__ int s_box[2][TRACK_BOXES_MAX][4];     // columns [0], [1]) and rows [2], [3]) of a box; empty behind n
    __shared__ long long s_q4[2][TRACK_BOXES_MAX];   // 4 q, or 0: no depth test
    __shared__ int s_n[2];
    __shared__ int s_votes[TRACK_BOXES_MAX * TRACK_VOTE_PITCH];
    const int tid = (int)threadIdx.x, lane = tid & 63, chunk = (int)blockIdx.x, b = (int)blockIdx.y;
    for (int k = tid; k < TRACK_BOXES_MAX * TRACK_VOTE_PITCH; k += TRACK_THREADS) s_votes[k] = 0;
    if (tid < 2 * TRACK_BOXES_MAX) {
        const int f = tid >> 6, i = tid & 63;
        const int32_t *nn = f ? a.n1 : a.n0;
        int n = nn ? nn[b] : a.M;
        n = n < 0 ? 0 : n > a.M ? a.M : n;
        if (i == 0) s_n[f] = n;
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        long long q4 = 0;
        if (i < n) {
            const size_t at = (size_t)b * a.M + i;
            const int32_t *p = (f ? a.boxes1 : a.boxes0) + at * 4;
            x0 = track_clamp(p[0], a.W), x1 = track_clamp((long long)p[0] + p[2], a.W);
            y0 = track_clamp(p[1], a.H), y1 = track_clamp((long long)p[1] + p[3], a.H);
            const int q = (f ? a.q1 : a.q0)[at];
            q4 = q <= 0 ? 0 : 4ll * q;
        }
        s_box[f][i][0] = x0, s_box[f][i][1] = x1, s_box[f][i][2] = y0, s_box[f][i][3] = y1;
        s_q4[f][i] = q4;
    }
    __syncthreads();

    const int cnt = a.counts[b];
    const int rows = cnt < 0 ? 0 : cnt < a.cap ? cnt : a.cap;
    const int i = chunk * TRACK_THREADS + tid;
    u64 w0 = 0, w1 = 0;
    if (i < rows) {
        const int32_t *m = a.matches + ((size_t)b * a.cap + (size_t)i) * 6;
        const int u0 = m[0], v0 = m[1], u1 = m[3], v1 = m[4];
        const long long d0 = m[2], d1 = m[5];
        if (d0 >= 1 && d0 <= FLOW_DQ_MAX) {
            const int n0 = s_n[0], n1 = s_n[1];
            for (int k = 0; k < n0; k++) {
                const long long q4 = s_q4[0][k];
                const bool in = u0 >= s_box[0][k][0] && u0 < s_box[0][k][1] && v0 >= s_box[0][k][2] && v0 < s_box[0][k][3];
                const long long e = d0 - q4;
                if (in && (q4 == 0 || (e >= -a.band_q && e <= a.band_q))) w0 |= 1ull << k;
            }
            if (w0) {
                for (int k = 0; k < n1; k++) {
                    const long long q4 = s_q4[1][k];
                    const bool in = u1 >= s_box[1][k][0] && u1 < s_box[1][k][1] && v1 >= s_box[1][k][2] && v1 < s_box[1][k][3];
                    const long long e = d1 - q4;
                    if (in && (q4 == 0 || (d1 > 0 && e >= -a.band_q && e <= a.band_q))) w1 |= 1ull << k;
                }
            }
        }
    }
    if (i < a.cap) {
        u64 *w = a.words + ((size_t)b * a.cap + (size_t)i) * 2;
        w[0] = w0, w[1] = w1;
    }

    u64 any0 = wave_or(w0);  // every lane of the workgroup gets here
    while (any0) {
        const int k = __builtin_ctzll(any0);
        any0 &= any0 - 1;
        const bool has = (w0 >> k) & 1;
        const int members = __popcll(__ballot(has));
        u64 any1 = wave_or(has ? w1 : 0ull);
        if (lane == 0) atomicAdd(&s_votes[k * TRACK_VOTE_PITCH + TRACK_BOXES_MAX], members);
        while (any1) {
            const int j = __builtin_ctzll(any1);
            any1 &= any1 - 1;
            const int n = __popcll(__ballot(has && ((w1 >> j) & 1)));
            if (lane == 0) atomicAdd(&s_votes[k * TRACK_VOTE_PITCH + j], n);
        }
    }
    __syncthreads();
    for (int k = tid; k < TRACK_BOXES_MAX * TRACK_VOTE_PITCH; k += TRACK_THREADS) {
        const int v = s_votes[k];
        if (v) {
            const int r = k / TRACK_VOTE_PITCH, j = k - r * TRACK_VOTE_PITCH;  // r < n0 <= M; j < n1 <= M, or the members
            atomicAdd(a.votes + ((size_t)b * a.M + r) * (a.M + 1) + (j == TRACK_BOXES_MAX ? a.M : j), v);
        }
    }
}

__global__ __launch_bounds__(64) void k_track_link(TrackArgs a) {
    __shared__ int s_votes[TRACK_BOXES_MAX * TRACK_VOTE_PITCH];
    const int i = (int)threadIdx.x, b = (int)blockIdx.x;
    for (int k = i; k < a.M * (a.M + 1); k += 64) s_votes[k] = a.votes[(size_t)b * a.M * (a.M + 1) + k];  // M (M + 1) <= 64 * 65
    __syncthreads();
    int best = 0, bj = 0, second = 0, members = 0;
    bool keep = false;
    if (i < a.M) {
        const int *row = s_votes + i * (a.M + 1);
        best = row[0];
        for (int j = 1; j < a.M; j++) {
            const int v = row[j];
            if (v > best) second = best, best = v, bj = j;
            else if (v > second) second = v;
        }
        members = row[a.M];
        keep = best >= a.min_votes && 256ll * best >= (long long)a.share * members;
    }
    const int kj = keep ? bj : -1;
    bool lose = false;
    for (int o = 0; o < 64; o++) {  // every lane of the wavefront gets here
        const int oj = __shfl(kj, o, 64), ov = __shfl(best, o, 64);
        if (keep && o != i && oj == bj && (ov > best || (ov == best && o < i))) lose = true;
    }
    if (i < a.M) {
        int32_t *l = a.link + ((size_t)b * a.M + i) * 4;
        l[0] = keep && !lose ? bj : -1, l[1] = best, l[2] = members, l[3] = second;
    }
}

__global__ __launch_bounds__(TRACK_THREADS) void k_track_sums(TrackArgs a) {
    __shared__ u64 s_sums[TRACK_BOXES_MAX][TRACK_SUM_WORDS];
    __shared__ int s_link[TRACK_BOXES_MAX];
    __shared__ int s_centre[TRACK_BOXES_MAX][3];
    const int tid = (int)threadIdx.x, chunk = (int)blockIdx.x, b = (int)blockIdx.y;
    for (int k = tid; k < TRACK_BOXES_MAX * TRACK_SUM_WORDS; k += TRACK_THREADS) s_sums[k / TRACK_SUM_WORDS][k % TRACK_SUM_WORDS] = 0ull;
    if (tid < TRACK_BOXES_MAX) {
        const bool live = tid < a.M;
        s_link[tid] = live ? a.link[((size_t)b * a.M + tid) * 4] : -1;
#pragma unroll
        for (int c = 0; c < 3; c++) s_centre[tid][c] = live && a.centre ? a.centre[((size_t)b * a.M + tid) * 3 + c] : 0;
    }
    __syncthreads();

    const bool gated = a.centre && a.gate_m > 0;
    const int cnt = a.counts[b];
    const int rows = cnt < 0 ? 0 : cnt < a.cap ? cnt : a.cap;
    const int i = chunk * TRACK_THREADS + tid;
    u64 feed = 0;
    long long val[13];  // ru, rv, rd, ru^2 + rv^2, m[3], m^2[3], p[3]
#pragma unroll
    for (int k = 0; k < 13; k++) val[k] = 0;
    long long mv[3] = {0, 0, 0};
    if (i < rows) {
        const u64 *w = a.words + ((size_t)b * a.cap + (size_t)i) * 2;
        const u64 w0 = w[0], w1 = w[1];
        for (u64 r = w0; r; r &= r - 1) {
            const int k = __builtin_ctzll(r), j = s_link[k];
            if (j >= 0 && ((w1 >> j) & 1)) feed |= 1ull << k;
        }
        if (feed) {
            const int32_t *m = a.matches + ((size_t)b * a.cap + (size_t)i) * 6;
            const int u0 = m[0], v0 = m[1], d0 = m[2], u1 = m[3], v1 = m[4], d1 = m[5];  // d0 in 1 .. 2^20: the match has a word
            bool inside = false;
            if (d1 >= 1 && d1 <= FLOW_DQ_MAX) {
                const FlowCamera &c = a.cam;
                double x, y, z;
                flow_point(c, a.poses + (size_t)b * 12, u0, v0, d0, x, y, z);  // the pose: the same address in every lane
                if (z > FLOW_Z_MIN) {  // false for NaN
                    const double xz = x / z, yz = y / z, bz = c.fb / z;
                    const double pu = floor(16.0 * (c.f * xz + c.cx) + 0.5), pv = floor(16.0 * (c.f * yz + c.cy) + 0.5), pd = floor(16.0 * bz + 0.5);
                    if (fabs(pu) <= TRACK_PIXEL_MAX && fabs(pv) <= TRACK_PIXEL_MAX && fabs(pd) <= TRACK_PIXEL_MAX) {  // false for NaN
                        inside = true;
                        const double dd = (double)d1;
                        const double X1[3] = {(((double)u1 - c.cx) * c.b16) / dd, (((double)v1 - c.cy) * c.b16) / dd, c.fb16 / dd};
                        const double Xc[3] = {x, y, z};  // x and y finite, z finite or +inf: no NaN below
                        const long long ru = track_clip(16ll * u1 - (long long)pu, TRACK_M_MAX), rv = track_clip(16ll * v1 - (long long)pv, TRACK_M_MAX),
                                        rd = track_clip((long long)d1 - (long long)pd, TRACK_M_MAX);
                        val[0] = ru, val[1] = rv, val[2] = rd, val[3] = ru * ru + rv * rv;
#pragma unroll
                        for (int k = 0; k < 3; k++) {
                            mv[k] = track_q(1024.0 * (X1[k] - Xc[k]), (double)TRACK_M_MAX);
                            val[4 + k] = mv[k], val[7 + k] = mv[k] * mv[k];
                            val[10 + k] = track_q(1024.0 * X1[k], (double)TRACK_P_MAX);
                        }
                    }
                }
            }
            if (!inside) feed = 0;
        }
    }

    for (u64 r = feed; r; r &= r - 1) {
        const int k = __builtin_ctzll(r);
        atomicAdd(&s_sums[k][1], 1ull);
        const long long g = a.gate_m;
        if (gated && !(llabs(mv[0] - s_centre[k][0]) <= g && llabs(mv[1] - s_centre[k][1]) <= g && llabs(mv[2] - s_centre[k][2]) <= g)) continue;
        atomicAdd(&s_sums[k][0], 1ull);
#pragma unroll
        for (int q = 0; q < 13; q++) atomicAdd(&s_sums[k][2 + q], (u64)val[q]);
    }
    __syncthreads();
    for (int k = tid; k < TRACK_BOXES_MAX * TRACK_SUM_WORDS; k += TRACK_THREADS) {
        const int r = k / TRACK_SUM_WORDS, q = k % TRACK_SUM_WORDS;
        const u64 v = s_sums[r][q];
        if (v && r < a.M) atomicAdd(a.sums + ((size_t)b * a.M + r) * TRACK_SUM_WORDS + q, v);
    }
}

}  // namespace

hipError_t launch_object_links(const TrackArgs &a, hipStream_t st) {
    if (a.B < 1 || a.B > 65535 || a.M < 1 || a.M > TRACK_BOXES_MAX || a.cap < 0 || a.cap > FLOW_CAPACITY_MAX) return hipErrorInvalidValue;
    const int words = a.M * (a.M + 1 > TRACK_SUM_WORDS ? a.M + 1 : TRACK_SUM_WORDS), stop = a.flags & TRACK_STOP_MASK;
    hipLaunchKernelGGL(k_track_clear, dim3((unsigned)((words + TRACK_THREADS - 1) / TRACK_THREADS), (unsigned)a.B), dim3(TRACK_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (a.n_chunks > 0 && stop < 3) {
        hipLaunchKernelGGL(k_track_votes, dim3((unsigned)a.n_chunks, (unsigned)a.B), dim3(TRACK_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    if (stop < 2) {
        hipLaunchKernelGGL(k_track_link, dim3((unsigned)a.B), dim3(64), 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    if (a.n_chunks > 0 && stop < 1) hipLaunchKernelGGL(k_track_sums, dim3((unsigned)a.n_chunks, (unsigned)a.B), dim3(TRACK_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
