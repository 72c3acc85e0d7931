// An occupancy frame matched against the world map over candidate poses: include/stereo_vision_hip.h (L), restated in stereo_vision/sv.py
// (occupancy_match).  Three kernels, no atomics on the results and none in floating point:
//
//   lists   a workgroup covers 4096 cells of one frame, a thread 16 of them, 256 apart.  Two passes over the bytes it keeps in registers:
//           ballots count the wavefront's state-2 and state-1 cells, one integer atomic per workgroup and kind reserves room in the frame's
//           list, and the second pass writes each kept cell at the wavefront's base + the ballot's prefix as fr | fc << 15 (both below
//           32768).  Occupied cells fill the list from its front, free cells from its back, so the state needs no bits and the scoring
//           loop no branch on it; with w_free == 0 free cells are not kept.  The order inside either part is free.
//
//   scores  a workgroup owns G = 1 << log_group candidates of one frame and all of that frame's list; thread t scores candidate
//           t % G over the list entries t / G, t / G + 256 / G, ...  The host picks G: 256 where batch x ceil(P / G) workgroups still fill
//           the chip, down to 1 - the candidate uniform per workgroup, the lanes striding over the list - for a single small window.
//           Either way every lane's doubles are one lookup: a candidate's pose sits in four registers of its lane.  The list is staged
//           1024 entries at a time in LDS as the doubles (Xf, Yf) - the conversion from the packed word is made once per workgroup, not
//           per lookup.  Per lookup the way into a cell that every reader of the map takes (occupancy_map_cells.h: four products, two
//           sums, the translation, the map's scale, floor, four comparisons in double) and one int16 load.  Sums in int32 per chunk (1024 x
//           32768 < 2^31), int64 across chunks.  The 256 / G partial sums of a candidate meet in an LDS tree; one thread stores its
//           (H, M), its counts and, where the best is wanted, the workgroup's maximum as one (score, lowest index) pair.
//
//   best    a workgroup per frame over its at most 2048 pairs.
//
// No workgroup waits for another; the list's counters are cleared by a memset node in front of the first kernel.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "map_match_kernels.h"
#include "occupancy_map_cells.h"

namespace sv {

__global__ __launch_bounds__(MAPMATCH_THREADS) void k_map_match_lists(MapMatchArgs a) {
    __shared__ uint32_t s_wave[2][4], s_base[2];
    const int b = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t cell0 = (size_t)blockIdx.x * MAPMATCH_COMPACT_CELLS;
    const uint8_t *st = a.state + (size_t)b * a.cap;
    const bool keep_free = a.w_free != 0;
    uint8_t v[MAPMATCH_COMPACT_ITEMS];
    uint32_t n2 = 0, n1 = 0;  // wave-uniform
#pragma unroll
    for (int k = 0; k < MAPMATCH_COMPACT_ITEMS; k++) {
        const size_t i = cell0 + (size_t)k * MAPMATCH_THREADS + tid;
        v[k] = i < a.cap ? st[i] : (uint8_t)0;
        n2 += (uint32_t)__popcll(__ballot(v[k] == 2));
        n1 += (uint32_t)__popcll(__ballot(keep_free && v[k] == 1));
    }
    if (lane == 0) s_wave[0][wave] = n2, s_wave[1][wave] = n1;
    __syncthreads();
    if (tid < 2) {
        const uint32_t n = s_wave[tid][0] + s_wave[tid][1] + s_wave[tid][2] + s_wave[tid][3];
        s_base[tid] = n ? atomicAdd(tid == 0 ? &a.headers[b].n_occ : &a.headers[b].n_free, n) : 0u;
    }
    __syncthreads();
    uint32_t at2 = s_base[0], at1 = s_base[1];
    for (int w = 0; w < wave; w++) at2 += s_wave[0][w], at1 += s_wave[1][w];
    uint32_t *list = a.lists + (size_t)b * a.cap;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int k = 0; k < MAPMATCH_COMPACT_ITEMS; k++) {
        const size_t i = cell0 + (size_t)k * MAPMATCH_THREADS + tid;
        const unsigned long long m2 = __ballot(v[k] == 2), m1 = __ballot(keep_free && v[k] == 1);
        const uint32_t word = (uint32_t)(i / (size_t)a.fcols) | (uint32_t)(i % (size_t)a.fcols) << 15;
        // every kept cell holds one slot: n_occ + n_free <= cap, so the two parts never meet
        if (v[k] == 2) list[at2 + (uint32_t)__popcll(m2 & below)] = word;
        else if (keep_free && v[k] == 1) list[a.cap - 1 - (at1 + (uint32_t)__popcll(m1 & below))] = word;
        at2 += (uint32_t)__popcll(m2), at1 += (uint32_t)__popcll(m1);
    }
}

// The higher score, at equal scores the lower index.
__device__ inline bool better(long long s, int i, long long s0, int i0) { return s > s0 || (s == s0 && i < i0); }

template <bool COUNT>
__global__ __launch_bounds__(MAPMATCH_THREADS) void k_map_match_scores(MapMatchArgs a) {
    __shared__ double s_x[MAPMATCH_CHUNK], s_y[MAPMATCH_CHUNK];
    __shared__ long long s_h[MAPMATCH_THREADS], s_m[MAPMATCH_THREADS];
    __shared__ int s_n2[MAPMATCH_THREADS], s_n1[MAPMATCH_THREADS];
    const int b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int G = 1 << a.log_group, c = tid & (G - 1), slice = tid >> a.log_group, slices = MAPMATCH_THREADS >> a.log_group;
    const int p = (int)blockIdx.x * G + c;
    const bool valid = p < a.P;
    double tx = 0.0, ty = 0.0, pc = 0.0, ps = 0.0;
    if (valid) {
        const double *pose = a.poses + ((size_t)b * a.P + p) * 4;
        tx = pose[0], ty = pose[1], pc = pose[2], ps = pose[3];
    }
    const uint32_t n2 = a.headers[b].n_occ, n1 = a.w_free != 0 ? a.headers[b].n_free : 0u, n = n2 + n1;
    const uint32_t *list = a.lists + (size_t)b * a.cap;
    long long H = 0, M = 0;
    int c2 = 0, c1 = 0;
    unsigned long long lookups = 0;

    // entry k of the staged chunk under this lane's pose -> the map's word, or no hit
    auto lookup = [&](int k, int &sum, int &hits) {
        double Xw, Yw;
        map_world(tx, ty, pc, ps, s_x[k], s_y[k], Xw, Yw);
        if (COUNT) lookups++;
        int r, cc;
        if (map_cell(a.m, map_grid(a.m, Xw), map_grid(a.m, Yw), r, cc)) {
            sum += a.logodds[(size_t)r * a.m.cols + cc];
            hits++;
        }
    };

    for (uint32_t base = 0; base < n; base += MAPMATCH_CHUNK) {
        const int m = (int)min((uint32_t)MAPMATCH_CHUNK, n - base);
        __syncthreads();  // the chunk before is read
        for (int k = tid; k < m; k += MAPMATCH_THREADS) {
            const uint32_t j = base + (uint32_t)k;
            const uint32_t word = j < n2 ? list[j] : list[a.cap - 1 - (j - n2)];
            const double kx = a.fr1 - (double)(word & 32767u), ky = a.fc1 - (double)(word >> 15 & 32767u);
            // 2 k + sgn(k): integers below 2^48, exact
            s_x[k] = (2.0 * kx + (kx > 0.0 ? 1.0 : kx < 0.0 ? -1.0 : 0.0)) * a.hf;
            s_y[k] = (2.0 * ky + (ky > 0.0 ? 1.0 : ky < 0.0 ? -1.0 : 0.0)) * a.hf;
        }
        __syncthreads();
        if (valid) {
            const int m2 = base < n2 ? (int)min((uint32_t)m, n2 - base) : 0;  // the chunk's occupied entries come first
            int h = 0, f = 0;
            int k = slice;
            for (; k < m2; k += slices) lookup(k, h, c2);
            for (; k < m; k += slices) lookup(k, f, c1);
            H += h, M += f;
        }
    }
    if (COUNT && lookups) atomicAdd(a.lookups, lookups);

    s_h[tid] = H, s_m[tid] = M, s_n2[tid] = c2, s_n1[tid] = c1;
    for (int s = slices >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (slice < s) {
            const int o = tid + (s << a.log_group);
            s_h[tid] += s_h[o], s_m[tid] += s_m[o], s_n2[tid] += s_n2[o], s_n1[tid] += s_n1[o];
        }
    }
    // thread t < G now holds candidate t's sums (it wrote them itself last)
    long long score = LLONG_MIN;
    int index = INT_MAX;
    if (slice == 0 && valid) {
        H = s_h[tid], M = s_m[tid];
        const size_t o = ((size_t)b * a.P + p) * 2;
        if (a.sums) {
            a.sums[o] = H, a.sums[o + 1] = M;
            a.counts[o] = s_n2[tid], a.counts[o + 1] = s_n1[tid];
        }
        score = (long long)a.w_occ * H - (long long)a.w_free * M, index = p;
    }
    if (!a.best) return;  // one value for the grid
    __syncthreads();
    s_h[tid] = score, s_n2[tid] = index;
    for (int s = MAPMATCH_THREADS >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s && better(s_h[tid + s], s_n2[tid + s], s_h[tid], s_n2[tid])) s_h[tid] = s_h[tid + s], s_n2[tid] = s_n2[tid + s];
    }
    if (tid == 0) {  // candidate blockIdx.x * G exists, so the pair is one
        MapMatchPartial *out = a.partials + (size_t)b * MAPMATCH_PARTIALS + blockIdx.x;
        out->score = s_h[0], out->index = s_n2[0], out->pad = 0;
    }
}

__global__ __launch_bounds__(MAPMATCH_THREADS) void k_map_match_best(MapMatchArgs a) {
    __shared__ long long s_s[MAPMATCH_THREADS];
    __shared__ int s_i[MAPMATCH_THREADS];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const MapMatchPartial *in = a.partials + (size_t)b * MAPMATCH_PARTIALS;
    long long score = LLONG_MIN;
    int index = INT_MAX;
    for (int g = tid; g < a.n_groups; g += MAPMATCH_THREADS)
        if (better(in[g].score, in[g].index, score, index)) score = in[g].score, index = in[g].index;
    s_s[tid] = score, s_i[tid] = index;
    for (int s = MAPMATCH_THREADS >> 1; s >= 1; s >>= 1) {
        __syncthreads();
        if (tid < s && better(s_s[tid + s], s_i[tid + s], s_s[tid], s_i[tid])) s_s[tid] = s_s[tid + s], s_i[tid] = s_i[tid + s];
    }
    if (tid == 0) a.best[b] = s_i[0], a.best_score[b] = s_s[0];
}

hipError_t launch_map_match(const MapMatchArgs &a, hipStream_t st, int stages) {
    hipError_t e = hipMemsetAsync(a.headers, 0, (size_t)a.B * sizeof(MapMatchHeader), st);
    if (e != hipSuccess) return e;
    const dim3 block(MAPMATCH_THREADS);
    const dim3 cells((unsigned)((a.cap + MAPMATCH_COMPACT_CELLS - 1) / MAPMATCH_COMPACT_CELLS), a.B);
    hipLaunchKernelGGL(k_map_match_lists, cells, block, 0, st, a);
    if (stages >= 2) {
        const dim3 groups(a.n_groups, a.B);
        if (a.lookups) hipLaunchKernelGGL(k_map_match_scores<true>, groups, block, 0, st, a);
        else hipLaunchKernelGGL(k_map_match_scores<false>, groups, block, 0, st, a);
    }
    if (stages >= 3 && a.best) hipLaunchKernelGGL(k_map_match_best, dim3(a.B), block, 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
