// The expected view of the world map from candidate poses: include/stereo_vision_hip.h (P), restated in stereo_vision/sv.py
// (occupancy_view).  Rays are cast through the map from every candidate, and the DISTINCT cells they see are counted by state.  Doubles
// place the origin and the ends of the rays - by occupancy_map_cells.h, as the match and the path check place their points -,
// everything after that is integers: the same bits whatever order the lanes take.
//
//   state    one pass over the map: the state of every cell (occupancy_map_state's: 0 unknown, 1 free, 2 occupied) as a byte of the
//            workspace.  Chunks of 16 cells: the wide loader (occupancy_map_cells.h: map_state16) and one 16-byte store where the inputs
//            are 16-byte aligned (the workspace always is); cell by cell elsewhere and in the cut chunk at the end.  The walk then loads
//            one byte per lookup, not six.
//
//   walk     a workgroup of 256 threads per candidate; its lanes stride over the rays.  The workgroup holds a bitmap of the (2 w + 1)^2
//            window of cells around its origin in LDS, rows padded to whole 32-bit words, w = the call's reach (or 254 under
//            sv_debug_view): zeroed, a barrier, then the walk.  A ray whose end lies more than `reach` cells from the origin on either
//            axis is invalid and walks nothing, and a ray's cells move monotonically from the origin to its end: every cell a ray marks
//            lies inside the window.  A visible cell is marked with an LDS atomicOr; the lane whose returned word lacked the bit is the
//            cell's first visitor and adds one to its private counter of the cell's state.  The three counters are summed over the
//            wavefront by shuffles (wave_ops.h) and over the four wavefronts through twelve LDS words.
//
//            The line is occupancy_ray_cells' (obstacle_end = False): step k is at r0 + floor((2 k dr + n) / (2 n)) with n = max(|dr|,
//            |dc|).  It is walked with a remainder per axis instead of a division per step (occupancy_map_cells.h: line_step), so a
//            coordinate moves by at most one per step.
//
//   best     a wavefront per group g: the largest score of its P candidates, ties to the lowest index, as one 64-bit key (score + 1 in
//            the high word, ~index in the low one) under wave_max.  map_match's better() compares separate pairs in an LDS ladder of its
//            own file; the packed key lets the shared reduction do it.
//
// No global atomic, no word that two workgroups of one launch share, no loop that waits: the ray loop runs at most `reach` steps, the
// ray stride at most 4 times.  Every map lookup is behind an inside test on the cell's integers; every LDS word is addressed by offsets
// in 0 .. 2 reach.  The shuffles run after the ray loop, where every lane has arrived; the barriers stand outside every branch that a
// thread of the workgroup could skip - an invalid candidate leaves as a whole workgroup before the first of them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "view_kernels.h"
#include "occupancy_map_cells.h"
#include "wave_ops.h"

namespace sv {

__global__ __launch_bounds__(VIEW_THREADS) void k_view_state(ViewArgs a) {
    const int64_t cells = (int64_t)a.m.rows * a.m.cols;
    const int64_t g = ((int64_t)blockIdx.x * VIEW_THREADS + threadIdx.x) * VIEW_CHUNK;
    if (g >= cells) return;  // no barrier in this kernel
    const bool wide_in = ((reinterpret_cast<uintptr_t>(a.logodds) | reinterpret_cast<uintptr_t>(a.last_seen)) & 15) == 0;
    if (wide_in && g + VIEW_CHUNK <= cells) {
        uint32_t w[4];
        map_state16(a.logodds + g, a.last_seen + g, a.occupied, a.free_, w);
        *reinterpret_cast<uint4 *>(a.state + g) = make_uint4(w[0], w[1], w[2], w[3]);  // g is a multiple of 16, the workspace 16-byte aligned
    } else {
        const int n = (int)min((int64_t)VIEW_CHUNK, cells - g);
        for (int k = 0; k < n; k++) a.state[g + k] = (uint8_t)map_state(a.logodds[g + k], a.last_seen[g + k], a.occupied, a.free_);
    }
}

__global__ __launch_bounds__(VIEW_THREADS) void k_view_walk(ViewArgs a) {
    extern __shared__ uint32_t s_seen[];  // [2 window + 1][row_words]
    __shared__ int32_t s_count[VIEW_THREADS / 64][3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cand = (int)blockIdx.x;
    const double *pose = a.poses + (size_t)cand * 4;
    const double tx = pose[0], ty = pose[1], pc = pose[2], ps = pose[3];
    uint8_t *status = a.status + (size_t)cand * a.n_rays;
    uint32_t *ends_out = reinterpret_cast<uint32_t *>(a.end_cells) + (size_t)cand * a.n_rays;  // a cell is one 4-byte word: (row, col) as two int16
    const uint32_t none = 0xFFFFFFFFu;                                                       // (-1, -1)

    // the origin: uniform over the workgroup
    const double gx0 = map_grid(a.m, tx), gy0 = map_grid(a.m, ty);
    int r0 = 0, c0 = 0;
    if (!(isfinite(tx) && isfinite(ty) && isfinite(pc) && isfinite(ps) && map_cell(a.m, gx0, gy0, r0, c0))) {  // the whole workgroup, before any barrier
        for (int j = tid; j < a.n_rays; j += VIEW_THREADS) status[j] = (uint8_t)VIEW_INVALID, ends_out[j] = none;
        if (tid == 0) {
            a.counts[(size_t)cand * 3] = 0, a.counts[(size_t)cand * 3 + 1] = 0, a.counts[(size_t)cand * 3 + 2] = 0;
            a.score[cand] = -1;
        }
        return;
    }

    const int W = a.window, row_words = (2 * W + 1 + 31) >> 5, n_words = (2 * W + 1) * row_words;
    for (int i = tid; i < n_words; i += VIEW_THREADS) s_seen[i] = 0;
    __syncthreads();

    int seen0 = 0, seen1 = 0, seen2 = 0;  // this lane's first visits, by state
    const double reach = (double)a.reach;
    for (int j = tid; j < a.n_rays; j += VIEW_THREADS) {
        double Xw, Yw;
        map_world(tx, ty, pc, ps, a.ends[2 * j], a.ends[2 * j + 1], Xw, Yw);
        const double gx1 = map_grid(a.m, Xw), gy1 = map_grid(a.m, Yw);
        const double ddr = gx0 - gx1, ddc = gy0 - gy1;  // the end cell minus the origin cell: rows and columns count against gx and gy
        // NaN fails the comparisons; an end further than reach cells away on an axis must not walk, whatever its direction: this bounds the window
        if (!(isfinite(gx1) && isfinite(gy1) && fabs(ddr) <= reach && fabs(ddc) <= reach)) {
            status[j] = (uint8_t)VIEW_INVALID, ends_out[j] = none;
            continue;
        }
        const int dr = (int)ddr, dc = (int)ddc;
        const int n = max(abs(dr), abs(dc)), two_n = 2 * n;
        int r = r0, c = c0, acc_r = n, acc_c = n, er = r0, ec = c0, unknown = 0, st = VIEW_FULL;
        for (int k = 0; k <= n; k++) {
            if (k > 0) {
                const int pr = r, pcol = c;
                line_step(acc_r, r, 2 * dr, two_n), line_step(acc_c, c, 2 * dc, two_n);
                if ((unsigned)r >= (unsigned)a.m.rows || (unsigned)c >= (unsigned)a.m.cols) {
                    st = VIEW_EDGE;
                    break;
                }
                if (r != pr && c != pcol) {  // a diagonal step: the two cells beside it.  (pr, pcol) is inside the map, so (pr, c) and (r, pcol) are too
                    if (a.state[(size_t)pr * a.m.cols + c] == 2 && a.state[(size_t)r * a.m.cols + pcol] == 2) {
                        st = VIEW_CORNER;
                        break;
                    }
                }
            }
            const uint32_t cell = a.state[(size_t)r * a.m.cols + c];
            const int wr = r - r0 + W, wc = c - c0 + W;  // 0 .. 2 W: |r - r0| <= |dr| <= reach <= W
            const uint32_t bit = 1u << (wc & 31);
            const uint32_t old = atomicOr(&s_seen[wr * row_words + (wc >> 5)], bit);
            if (!(old & bit)) seen0 += cell == 0, seen1 += cell == 1, seen2 += cell == 2;
            er = r, ec = c;
            if (k > 0) {
                if (cell == 2) {
                    st = VIEW_HIT;
                    break;
                }
                if (cell == 0 && a.max_unknown > 0 && ++unknown == a.max_unknown) {
                    st = VIEW_UNKNOWN;
                    break;
                }
            }
        }
        status[j] = (uint8_t)st, ends_out[j] = (uint32_t)(uint16_t)er | (uint32_t)(uint16_t)ec << 16;
    }

    // every lane is here: the loop above has no exit of its own
    const int n0 = wave_sum(seen0), n1 = wave_sum(seen1), n2 = wave_sum(seen2);
    if (lane == 0) s_count[wave][0] = n0, s_count[wave][1] = n1, s_count[wave][2] = n2;
    __syncthreads();
    if (tid < 3) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < VIEW_THREADS / 64; w++) total += s_count[w][tid];
        a.counts[(size_t)cand * 3 + tid] = total;
        if (tid == 0) a.score[cand] = total;
    }
}

__global__ __launch_bounds__(VIEW_THREADS) void k_view_best(ViewArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int g = (int)blockIdx.x * (VIEW_THREADS / 64) + ((int)threadIdx.x >> 6);
    if (g >= a.G) return;  // a whole wavefront; no barrier in this kernel
    const int32_t *score = a.score + (size_t)g * a.P;
    long long key = -1;  // below every candidate's: a score is >= -1, so a key is >= 0
    for (int p = lane; p < a.P; p += 64) {
        const long long k = (long long)(score[p] + 1) << 32 | (long long)(0xFFFFFFFFu - (uint32_t)p);
        key = k > key ? k : key;
    }
    key = wave_max(key);  // P >= 1: lane 0 had a candidate
    if (lane == 0) a.best[g] = (int32_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFll)), a.best_score[g] = (int32_t)(key >> 32) - 1;
}

hipError_t launch_view(const ViewArgs &a, hipStream_t st, int stages) {
    const int64_t chunks = ((int64_t)a.m.rows * a.m.cols + VIEW_CHUNK - 1) / VIEW_CHUNK;
    hipLaunchKernelGGL(k_view_state, dim3((unsigned)((chunks + VIEW_THREADS - 1) / VIEW_THREADS)), dim3(VIEW_THREADS), 0, st, a);
    if (stages >= 2) {
        const int W = a.window;
        const size_t lds = (size_t)(2 * W + 1) * ((2 * W + 1 + 31) >> 5) * sizeof(uint32_t);  // at most 509 x 16 words = 32 576 bytes
        hipLaunchKernelGGL(k_view_walk, dim3(a.G * a.P), dim3(VIEW_THREADS), lds, st, a);
    }
    if (stages >= 3) hipLaunchKernelGGL(k_view_best, dim3((a.G + VIEW_THREADS / 64 - 1) / (VIEW_THREADS / 64)), dim3(VIEW_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
