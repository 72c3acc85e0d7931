// Occupancy and elevation grids from disparity maps, obstacle labels and free space: include/stereo_vision_hip.h (J), restated in
// stereo_vision/sv.py (occupancy_grid).  Four kernels on one stream, the outputs are the accumulators:
//
//   clear     counts 0, h_lo INT_MAX, h_hi -1 - one 16-byte store per cell - and n_rays 0: nothing is assumed of the caller's memory
//   evidence  the top view's disparity front end (reproject.h's "d1" form, the strict range test, the cell arithmetic and its
//             argument why every in-range point lands inside the grid: top_view_kernels.hip) on the pixels with d > 0 and label 1
//             or 2; h = min(trunc((Z - z0) * z_scale), 65535) - Z > z0, so nothing is negative, and a product that is +inf
//             (z0 = -inf) saturates.  A cell takes atomicAdd on one of two counts, atomicMin on h_lo and atomicMax on h_hi: integers,
//             so the order does not matter.  With `combine` the lanes of a wavefront are split into runs of equal cells (neighbouring
//             pixels mostly share one), a segmented scan leaves the run's two counts, its minimum and its maximum in its last lane,
//             and only that lane issues atomics - at most four per run instead of three per pixel.
//   rays      a lane per image column.  The end of its sight line is the column's obstacle base (free_row >= 0: arithmetic on three
//             numbers, no pixel is read) or its topmost ground pixel - rows walked from 0, a wavefront reads 64 neighbouring label
//             bytes per step.  Step k of the line from cell (r0, c0) to (r1, c1) is at (r0 + (2 k dr + n) / (2 n), c0 + (2 k dc + n) /
//             (2 n)), floor division, n = max(|dr|, |dc|): a closed form in k, monotone per axis, so the steps inside the grid are one
//             interval, found per axis from  n (2 lo - 1) <= 2 k da <= n (2 hi + 1) - 1  (lo = -a0, hi = size - 1 - a0), and the walk
//             takes at most max(rows, cols) + 1 steps whatever the end.  Between steps the quotient and remainder of each axis are
//             carried along (occupancy_map_cells.h: line_step, the world map's view walks the same line), so the loop holds no division.
//             64-bit range: |trunc(X s)| < 2^24 for both ends, so |dr|, |dc|, n < 2^25; a line whose span misses the grid on an axis
//             is dropped first, which leaves |a0| < 2^25 + 2^15 and every product below 2^54.
//   finalize  h_lo of a cell without evidence becomes -1; state = 2 iff n_obstacle >= min_obstacle, else 1 iff n_ground >= min_ground
//             or n_rays >= min_rays, else 0.
//
// No workgroup waits for another: each kernel's blocks only add into cells, and the stream orders the kernels.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "occupancy_kernels.h"
#include "occupancy_map_cells.h"
#include "wave_ops.h"

namespace sv {

__global__ __launch_bounds__(256) void k_occupancy_clear(OccupancyArgs a) {
    const size_t n = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t cell = (size_t)blockIdx.y * n + i;
    reinterpret_cast<int4 *>(a.cells)[cell] = make_int4(0, 0, INT_MAX, -1);
    a.n_rays[cell] = 0;
}

template <bool COMBINE, bool COUNT_ATOMICS>
__global__ __launch_bounds__(256) void k_occupancy_evidence(OccupancyArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, b = blockIdx.z;
    int cell = -1;      // -1: no evidence
    uint32_t cnt = 0;   // ground pixels in the low half, obstacle pixels in the high half
    int lo = 0, hi = 0;
    if (i < a.W) {
        const size_t p = ((size_t)b * a.H + j) * a.W + i;
        const float dv = a.disp[p];
        const uint32_t lab = a.labels[p];
        if (dv > 0.f && (lab == 1u || lab == 2u)) {
            double X, Y, Z;
            sv_reproject_point(a.rp, (double)i, (double)j, (double)dv, X, Y, Z);
            if (X > a.x0 && X < a.x1 && Y > a.y0 && Y < a.y1 && Z > a.z0 && Z < a.z1) {
                const int row = (int)(a.x1s - trunc(X * a.s)), col = (int)(a.y1s - trunc(Y * a.s));
                // always true (top_view_kernels.hip's argument); kept so that no input can ever address outside the grid
                if ((unsigned)row < (unsigned)a.rows && (unsigned)col < (unsigned)a.cols) {
                    cell = row * a.cols + col;
                    const double t = (Z - a.z0) * a.zs;  // > 0, maybe +inf
                    lo = hi = t >= (double)OCC_H_MAX ? (int)OCC_H_MAX : (int)t;
                    cnt = lab == 1u ? 1u : 0x10000u;
                }
            }
        }
    }
    bool issue = cell >= 0;
    if (COMBINE) {  // every lane of the block gets here: no early return above
        const WaveRun run = wave_run(cell);
        wave_run_scan(run, [&](int d, bool take) {  // the tail holds the run's counts, minimum and maximum
            const uint32_t c = __shfl_up(cnt, d);
            const int l = __shfl_up(lo, d), h = __shfl_up(hi, d);
            if (take) cnt += c, lo = min(lo, l), hi = max(hi, h);
        });
        issue = issue && run.tail;
    }
    if (issue) {
        int32_t *c = a.cells + 4 * (((size_t)b * a.rows) * a.cols + cell);
        const int g = (int)(cnt & 0xffffu), o = (int)(cnt >> 16);
        if (g) atomicAdd(c, g);
        if (o) atomicAdd(c + 1, o);
        atomicMin(c + 2, lo);
        atomicMax(c + 3, hi);
        if (COUNT_ATOMICS) atomicAdd(a.atomics, (unsigned long long)(2 + (g ? 1 : 0) + (o ? 1 : 0)));
    }
}

// floor(a / b) and ceil(a / b) for either sign, b != 0
__device__ __forceinline__ long long floor_div(long long a, long long b) {
    const long long q = a / b;
    return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q;
}
__device__ __forceinline__ long long ceil_div(long long a, long long b) { return -floor_div(-a, b); }

// The steps of one axis that stay inside 0 .. size - 1, cut into [k_lo, k_hi]; false: none.
__device__ __forceinline__ bool clip_axis(long long a0, long long da, long long n, int size, long long &k_lo, long long &k_hi) {
    const long long lo = n * (2 * (-a0) - 1), hi = n * (2 * ((long long)size - 1 - a0) + 1) - 1;
    if (da == 0) return lo <= 0 && 0 <= hi;
    if (da > 0) {
        k_lo = max(k_lo, ceil_div(lo, 2 * da));
        k_hi = min(k_hi, floor_div(hi, 2 * da));
    } else {
        k_lo = max(k_lo, ceil_div(hi, 2 * da));
        k_hi = min(k_hi, floor_div(lo, 2 * da));
    }
    return true;
}

__global__ __launch_bounds__(64) void k_occupancy_rays(OccupancyArgs a) {
    const int u = (int)blockIdx.x * 64 + (int)threadIdx.x, b = blockIdx.y;
    if (u >= a.W) return;
    const int fr = a.free_row[(size_t)b * a.W + u];
    const bool obstacle = fr >= 0;
    double v, d;
    if (obstacle) {
        v = (double)fr, d = (double)a.free_disp[(size_t)b * a.W + u];
    } else {
        const size_t frame = (size_t)b * a.H * a.W + u;
        int top = -1;
        float dv = 0.f;
        for (int r = 0; r < a.H; r++) {
            if (a.labels[frame + (size_t)r * a.W] != 1) continue;
            dv = a.disp[frame + (size_t)r * a.W];
            if (dv > 0.f) {
                top = r;
                break;
            }
        }
        if (top < 0) return;  // no ground in the column: no sight line
        v = (double)top, d = (double)dv;
    }
    double X, Y, Z;
    sv_reproject_point(a.rp, (double)u, v, d, X, Y, Z);
    if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) return;
    const double tx = trunc(X * a.s), ty = trunc(Y * a.s);  // +-inf where the product overflows
    if (!(fabs(tx) < (double)OCC_CELL_MAX && fabs(ty) < (double)OCC_CELL_MAX)) return;
    const long long r0 = a.r0, c0 = a.c0, r1 = (long long)(a.x1s - tx), c1 = (long long)(a.y1s - ty);
    const long long dr = r1 - r0, dc = c1 - c0;
    const long long n = max(dr < 0 ? -dr : dr, dc < 0 ? -dc : dc);
    if (max(r0, r1) < 0 || min(r0, r1) > a.rows - 1 || max(c0, c1) < 0 || min(c0, c1) > a.cols - 1) return;
    int32_t *out = a.n_rays + ((size_t)b * a.rows) * a.cols;
    if (n == 0) {  // both ends in one cell, inside the grid by the test above: a ground end counts it, an obstacle end nothing
        if (!obstacle) atomicAdd(out + (size_t)r0 * a.cols + (size_t)c0, 1);
        return;
    }
    long long k_lo = 0, k_hi = obstacle ? n - 1 : n;
    if (!clip_axis(r0, dr, n, a.rows, k_lo, k_hi) || !clip_axis(c0, dc, n, a.cols, k_lo, k_hi)) return;
    const long long two_n = 2 * n;
    long long qr = floor_div(2 * k_lo * dr + n, two_n), qc = floor_div(2 * k_lo * dc + n, two_n);
    long long mr = 2 * k_lo * dr + n - qr * two_n, mc = 2 * k_lo * dc + n - qc * two_n;  // remainders in 0 .. 2 n - 1
    for (long long k = k_lo; k <= k_hi; k++) {
        const long long r = r0 + qr, c = c0 + qc;
        // always true by the clip; kept so that no input can ever address outside the grid
        if ((unsigned long long)r < (unsigned long long)a.rows && (unsigned long long)c < (unsigned long long)a.cols)
            atomicAdd(out + (size_t)r * a.cols + (size_t)c, 1);
        line_step(mr, qr, 2 * dr, two_n), line_step(mc, qc, 2 * dc, two_n);
    }
}

__global__ __launch_bounds__(256) void k_occupancy_finalize(OccupancyArgs a) {
    const size_t n = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t cell = (size_t)blockIdx.y * n + i;
    const int4 c = reinterpret_cast<const int4 *>(a.cells)[cell];
    if (c.w < 0) a.cells[4 * cell + 2] = -1;
    if (a.state) a.state[cell] = c.y >= a.min_obstacle ? 2 : ((c.x >= a.min_ground || a.n_rays[cell] >= a.min_rays) ? 1 : 0);
}

static dim3 cell_grid(const OccupancyArgs &a, int batch) { return dim3((unsigned)(((size_t)a.rows * a.cols + 255) / 256), batch); }

hipError_t launch_occupancy_clear(const OccupancyArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_occupancy_clear, cell_grid(a, batch), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_occupancy_evidence(const OccupancyArgs &a, int batch, bool combine, hipStream_t st) {
    const dim3 grid((a.W + 255) / 256, a.H, batch), block(256);
    if (combine) {
        if (a.atomics) hipLaunchKernelGGL((k_occupancy_evidence<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_occupancy_evidence<true, false>), grid, block, 0, st, a);
    } else {
        if (a.atomics) hipLaunchKernelGGL((k_occupancy_evidence<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_occupancy_evidence<false, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_occupancy_rays(const OccupancyArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_occupancy_rays, dim3((a.W + 63) / 64, batch), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_occupancy_finalize(const OccupancyArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_occupancy_finalize, cell_grid(a, batch), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
