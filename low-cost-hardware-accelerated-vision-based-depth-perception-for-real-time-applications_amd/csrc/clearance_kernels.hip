// The obstacle-clearance field of the world map and the footprint check of candidate paths against it: include/stereo_vision_hip.h (M),
// restated in stereo_vision/sv.py (occupancy_clearance, clearance_paths).  Integers behind the source test and behind floor(): minima and
// counts, which do not depend on any order.  No atomics on the results, none in floating point.
//
//   cols    a lane per column, a workgroup 256 columns x a strip of 64 rows.  The lane runs one counter down the R rows above the strip
//           and one up the R rows below it, keeps the strip's own source flags as one 64-bit word - the only place the source test is
//           made - and reads each cell's distance to the nearest set bit above and below off that word (clz / ffs), falling back on the
//           two counters where the word has none.  g = that distance in rows, 255 beyond R; one byte stored per cell, nothing read back.
//
//   rows    a workgroup owns 8 rows x 256 columns and stages g for them with R columns on both sides in LDS (255 outside the map: the
//           edge is no obstacle).  A lane per cell walks dc = 0, +-1, +-2, ... and keeps best = min(best, dc^2 + g^2); a wavefront stops
//           as soon as dc^2 >= best in all of its lanes - nothing further out can win - so free space pays 2 R + 1 taps and the
//           neighbourhood of obstacles a few.  255^2 = 65025 > 254^2 >= R^2: a column without a source needs no branch, it loses to the
//           final best > R^2 -> 65535.
//
//   fused   both passes in one kernel over 64 x 64 cells with a halo of R <= 32 all round: the flags of (64 + 2 R)^2 cells in LDS, a
//           thread per staged column for the two counters in place, then the row walk above.  The alternative the host may choose for
//           small R (clearance.cpp).
//
//   paths   a wavefront per path, its lanes striding over the n_steps x n_discs lookups with the step as the slow index, so that a
//           lane meets its steps in rising order; the world point and its cell by occupancy_map_cells.h, the match's very functions;
//           three wave reductions by shuffle and one store per path and output.  The discs arrive by value and are staged in LDS once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "clearance_kernels.h"
#include "occupancy_map_cells.h"
#include "wave_ops.h"

namespace sv {

__device__ inline bool clearance_source(const ClearanceArgs &a, size_t i) { return (int)a.logodds[i] >= a.t_occ || (a.unknown && a.last_seen[i] < 0); }

// One more row without a source on a counter that stops counting beyond R.
__device__ inline int clearance_step(int cnt, bool source, int R) { return source ? 0 : cnt >= R ? (int)CLEARANCE_NONE : cnt + 1; }

__global__ __launch_bounds__(CLEARANCE_THREADS) void k_clearance_cols(ClearanceArgs a) {
    const int c = (int)blockIdx.x * CLEARANCE_THREADS + (int)threadIdx.x;
    if (c >= a.cols) return;  // no barrier in this kernel
    const int R = a.R, r0 = (int)blockIdx.y * CLEARANCE_STRIP, r1 = min(a.rows, r0 + CLEARANCE_STRIP), n = r1 - r0;
    const size_t cols = (size_t)a.cols;
    int above = CLEARANCE_NONE, below = CLEARANCE_NONE;  // rows from r0 - 1 up, and from r1 down, to the nearest source: < R, or none
    for (int r = max(0, r0 - R); r < r0; r++) above = clearance_step(above, clearance_source(a, (size_t)r * cols + c), R);
    for (int r = min(a.rows - 1, r1 - 1 + R); r >= r1; r--) below = clearance_step(below, clearance_source(a, (size_t)r * cols + c), R);
    unsigned long long flags = 0;
    for (int i = 0; i < n; i++) flags |= (unsigned long long)clearance_source(a, (size_t)(r0 + i) * cols + c) << i;
    for (int i = 0; i < n; i++) {
        const unsigned long long upto = flags & (~0ull >> (63 - i)), from = flags >> i;
        const int up = upto ? i - (63 - __clzll((long long)upto)) : above == CLEARANCE_NONE ? 1 << 20 : above + i + 1;
        const int down = from ? __ffsll((unsigned long long)from) - 1 : below == CLEARANCE_NONE ? 1 << 20 : below + (n - i);
        const int d = min(up, down);
        a.g[(size_t)(r0 + i) * cols + c] = (uint8_t)(d > R ? (int)CLEARANCE_NONE : d);
    }
}

// The row walk of one cell over staged bytes: centre[-R .. R] are readable for every lane, valid or not.  -> d2 of the cell.
template <bool COUNT>
__device__ inline uint32_t clearance_walk(const uint8_t *centre, int R, bool early_exit, bool valid, unsigned long long &taps) {
    const uint32_t g0 = centre[0];
    uint32_t best = valid ? g0 * g0 : 0u;  // a lane without a cell never holds its wavefront back
    if (COUNT && valid) taps++;
    uint32_t dc2 = 1;
    for (int dc = 1; dc <= R; dc++) {
        if (early_exit && __ballot(dc2 < best) == 0ull) break;  // wave-uniform: everything further out is >= dc^2 >= best
        const uint32_t p = centre[dc], q = centre[-dc];
        best = min(best, min(p * p, q * q) + dc2);
        if (COUNT && valid) taps += 2;
        dc2 += 2u * (uint32_t)dc + 1u;
    }
    return best > (uint32_t)(R * R) ? (uint32_t)CLEARANCE_FAR : best;
}

template <bool COUNT>
__global__ __launch_bounds__(CLEARANCE_THREADS) void k_clearance_rows(ClearanceArgs a) {
    __shared__ uint8_t s_g[CLEARANCE_TILE_ROWS * (CLEARANCE_THREADS + 2 * CLEARANCE_MAX_R)];
    const int tid = (int)threadIdx.x, R = a.R, W = CLEARANCE_THREADS + 2 * R;
    const int c0 = (int)blockIdx.x * CLEARANCE_THREADS, r0 = (int)blockIdx.y * CLEARANCE_TILE_ROWS, n = min((int)CLEARANCE_TILE_ROWS, a.rows - r0);
    for (int rr = 0; rr < n; rr++) {
        const uint8_t *row = a.g + (size_t)(r0 + rr) * a.cols;
        for (int x = tid; x < W; x += CLEARANCE_THREADS) {
            const int col = c0 - R + x;
            s_g[rr * W + x] = col >= 0 && col < a.cols ? row[col] : (uint8_t)CLEARANCE_NONE;
        }
    }
    __syncthreads();
    const int c = c0 + tid;
    const bool valid = c < a.cols;
    unsigned long long taps = 0;
    for (int rr = 0; rr < n; rr++) {
        const uint32_t best = clearance_walk<COUNT>(s_g + rr * W + R + tid, R, a.early_exit != 0, valid, taps);
        if (valid) a.d2[(size_t)(r0 + rr) * a.cols + c] = (uint16_t)best;
    }
    if (COUNT && taps) atomicAdd(a.taps, taps);
}

template <bool COUNT>
__global__ __launch_bounds__(CLEARANCE_THREADS) void k_clearance_fused(ClearanceArgs a) {
    enum { SIDE = CLEARANCE_FUSED_TILE + 2 * CLEARANCE_FUSED_MAX_R };  // 128: two staged rows per sweep of the workgroup
    __shared__ uint8_t s_g[SIDE * SIDE];
    const int tid = (int)threadIdx.x, R = a.R, W = CLEARANCE_FUSED_TILE + 2 * R;
    const int c0 = (int)blockIdx.x * CLEARANCE_FUSED_TILE, r0 = (int)blockIdx.y * CLEARANCE_FUSED_TILE;
    {
        const int x = tid & (SIDE - 1), col = c0 - R + x;
        if (x < W)
            for (int y = tid / SIDE; y < W; y += CLEARANCE_THREADS / SIDE) {
                const int r = r0 - R + y;
                const bool in = r >= 0 && r < a.rows && col >= 0 && col < a.cols;
                s_g[y * W + x] = in && clearance_source(a, (size_t)r * a.cols + col) ? (uint8_t)0 : (uint8_t)CLEARANCE_NONE;
            }
    }
    __syncthreads();
    if (tid < W) {  // a staged column each: the counter down, then up, in place; a byte is 0 exactly on a source throughout
        int cnt = CLEARANCE_NONE;
        for (int y = 0; y < W; y++) {
            cnt = clearance_step(cnt, s_g[y * W + tid] == 0, R);
            s_g[y * W + tid] = (uint8_t)cnt;
        }
        cnt = CLEARANCE_NONE;
        for (int y = W - 1; y >= 0; y--) {
            const int down = s_g[y * W + tid];
            cnt = clearance_step(cnt, down == 0, R);
            s_g[y * W + tid] = (uint8_t)min(down, cnt);
        }
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, c = c0 + lane;
    const bool valid = c < a.cols;
    unsigned long long taps = 0;
    for (int rr = wave; rr < CLEARANCE_FUSED_TILE && r0 + rr < a.rows; rr += CLEARANCE_THREADS / 64) {  // wave-uniform bounds
        const uint32_t best = clearance_walk<COUNT>(s_g + (R + rr) * W + R + lane, R, a.early_exit != 0, valid, taps);
        if (valid) a.d2[(size_t)(r0 + rr) * a.cols + c] = (uint16_t)best;
    }
    if (COUNT && taps) atomicAdd(a.taps, taps);
}

__global__ __launch_bounds__(CLEARANCE_THREADS) void k_clearance_paths(ClearancePathsArgs a, ClearanceDiscs discs) {
    __shared__ double s_px[CLEARANCE_MAX_DISCS], s_py[CLEARANCE_MAX_DISCS];
    __shared__ int32_t s_r2[CLEARANCE_MAX_DISCS];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (tid < a.n_discs) s_px[tid] = discs.px[tid], s_py[tid] = discs.py[tid], s_r2[tid] = discs.r2[tid];
    __syncthreads();
    const int path = (int)blockIdx.x * (CLEARANCE_THREADS / 64) + (tid >> 6);
    if (path >= a.n_paths) return;  // a whole wavefront, behind the only barrier
    const double *poses = a.poses + (size_t)path * a.n_steps * 4;
    const int total = a.n_steps * a.n_discs;  // <= 65535 x 64
    const int step_q = 64 / a.n_discs, step_r = 64 % a.n_discs;
    int step = lane / a.n_discs, k = lane % a.n_discs;
    int first = a.n_steps, least = CLEARANCE_FAR, outside = 0;
    for (int i = lane; i < total; i += 64) {
        const double tx = poses[(size_t)step * 4], ty = poses[(size_t)step * 4 + 1], pc = poses[(size_t)step * 4 + 2], ps = poses[(size_t)step * 4 + 3];
        double Xw, Yw;
        map_world(tx, ty, pc, ps, s_px[k], s_py[k], Xw, Yw);
        int r, cc;
        if (map_cell(a.m, map_grid(a.m, Xw), map_grid(a.m, Yw), r, cc)) {
            const int v = a.d2[(size_t)r * a.m.cols + cc];
            least = min(least, v);
            if (v <= s_r2[k]) first = min(first, step);
        } else {
            outside++;
        }
        step += step_q, k += step_r;
        if (k >= a.n_discs) k -= a.n_discs, step++;
    }
    first = wave_min(first), least = wave_min(least), outside = wave_sum(outside);
    if (lane == 0) a.first_hit[path] = first, a.min_d2[path] = least, a.n_outside[path] = outside;
}

hipError_t launch_clearance(const ClearanceArgs &a, hipStream_t st, bool fused, int passes) {
    const dim3 block(CLEARANCE_THREADS);
    if (fused) {
        const dim3 grid((a.cols + CLEARANCE_FUSED_TILE - 1) / CLEARANCE_FUSED_TILE, (a.rows + CLEARANCE_FUSED_TILE - 1) / CLEARANCE_FUSED_TILE);
        if (a.taps) hipLaunchKernelGGL(k_clearance_fused<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_clearance_fused<false>, grid, block, 0, st, a);
        return hipGetLastError();
    }
    const unsigned across = (a.cols + CLEARANCE_THREADS - 1) / CLEARANCE_THREADS;
    if (passes & 1) hipLaunchKernelGGL(k_clearance_cols, dim3(across, (a.rows + CLEARANCE_STRIP - 1) / CLEARANCE_STRIP), block, 0, st, a);
    if (passes & 2) {
        const dim3 grid(across, (a.rows + CLEARANCE_TILE_ROWS - 1) / CLEARANCE_TILE_ROWS);
        if (a.taps) hipLaunchKernelGGL(k_clearance_rows<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(k_clearance_rows<false>, grid, block, 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_clearance_paths(const ClearancePathsArgs &a, const ClearanceDiscs &discs, hipStream_t st) {
    hipLaunchKernelGGL(k_clearance_paths, dim3((a.n_paths + CLEARANCE_THREADS / 64 - 1) / (CLEARANCE_THREADS / 64)), dim3(CLEARANCE_THREADS), 0, st, a, discs);
    return hipGetLastError();
}

}  // namespace sv
