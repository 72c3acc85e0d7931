// Bird's-eye view (top view) of point clouds: the reference's points_2_top_view helper (stereo_vision/sv.py:87-134), restated in
// stereo_vision/sv.py and specified in include/stereo_vision_hip.h (D).  One rasteriser core behind two front ends: a point is loaded
// from an f64 cloud, or computed in registers from a disparity map with reproject.h's arithmetic (the f64 cloud is never written).
//
//   in range    x0 < X < x1 && y0 < Y < y1 && z0 < Z < z1 (strict IEEE compares: NaN and +-inf never pass)
//   cell        row = trunc(x1 s) - trunc(X s), col = trunc(y1 s) - trunc(Y s), products in double
//   value       dist = sqrt(X*X + Y*Y) (no FMA: -ffp-contract=off; correctly rounded sqrt),
//               (uint8) trunc(((max_dist - dist) / max_dist) * 255), 0 where that is negative
//   reference   the value of the in-range point with the largest flat index n in the cell (numpy's last-writer order);
//               atomicMax on the key ((n + 1) << 8) | value, then the low byte - max is order-independent, so the grid is
//               bitwise reproducible
//   count       atomicAdd of the number of in-range points per cell
//
// Why every in-range point lands inside the grid (x shown, y alike): x0, x1 and s are integers with |x| s < 2^53, so x0 s and x1 s are
// exact doubles.  x0 < X < x1 and a correctly rounded product is monotone, so x0 s <= fl(X s) <= x1 s (equality only by rounding).
// trunc is monotone and leaves integers alone, so x0 s <= trunc(X s) <= x1 s, and row = x1 s - trunc(X s) lies in [0, (x1 - x0) s] =
// [0, rows - 1]; the difference of two integers below 2^53 is exact.
//
// Atomics: pixels next to each other in a row mostly fall in the same cell, above all in the far field.  With `combine` the lanes of
// a wavefront are split into runs of equal cells and only the last lane of a run issues the atomic: in reference mode its key is the
// run's largest (n grows with the lane), in count mode it adds the run's length (from a ballot of the run heads).  On KITTI this cuts
// the atomics to a third and the time to 0.3x.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "top_view_kernels.h"
#include "wave_ops.h"

namespace sv {

template <int SRC, int MODE, bool COMBINE, bool COUNT_ATOMICS>
__global__ __launch_bounds__(256) void k_top_view(TopViewArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y, b = blockIdx.z;
    int cell = -1;  // -1: no point, or out of range
    uint32_t value = 0;
    if (i < a.W) {
        double X, Y, Z;
        bool ok = true;
        if (SRC == TV_SRC_POINTS) {
            const double *p = a.points + 3 * ((size_t)b * a.W + i);
            X = p[0], Y = p[1], Z = p[2];
        } else {
            const float dv = a.disp[((size_t)b * a.H + j) * a.W + i];
            double d;
            if (SRC == TV_SRC_DMAP) {
                d = (double)sv_dmap_u8(dv);
            } else {
                d = (double)dv;
                ok = dv > 0.f;
            }
            if (ok) sv_reproject_point(a.rp, (double)i, (double)j, d, X, Y, Z);
        }
        if (ok && X > a.x0 && X < a.x1 && Y > a.y0 && Y < a.y1 && Z > a.z0 && Z < a.z1) {
            const int row = (int)(a.x1s - trunc(X * a.s)), col = (int)(a.y1s - trunc(Y * a.s));
            // always true by the argument above; kept so that no input can ever address outside the grid
            if ((unsigned)row < (unsigned)a.rows && (unsigned)col < (unsigned)a.cols) cell = row * a.cols + col;
            if (MODE == TV_MODE_REFERENCE) {
                const double dist = sqrt(X * X + Y * Y);
                const double q = ((a.max_dist - dist) / a.max_dist) * 255.0;
                value = q > 0.0 ? (uint32_t)q : 0u;  // q <= 255; negative only where dist > max_dist (documented deviation)
            }
        }
    }
    const size_t base = ((size_t)b * a.rows) * a.cols;
    bool issue = cell >= 0;
    int count = 1;
    if (COMBINE) {  // every lane of the block gets here: no early return above
        const WaveRun run = wave_run(cell);
        issue = issue && run.tail;
        if (MODE == TV_MODE_COUNT) count = (int)__lane_id() - run.head_lane + 1;  // the run's length
    }
    if (issue) {
        if (MODE == TV_MODE_REFERENCE) {
            const int n = SRC == TV_SRC_POINTS ? i : j * a.W + i;
            const unsigned long long key = ((unsigned long long)(n + 1) << 8) | value;
            atomicMax(static_cast<unsigned long long *>(a.grid) + base + cell, key);
        } else {
            atomicAdd(static_cast<int *>(a.grid) + base + cell, count);
        }
        if (COUNT_ATOMICS) atomicAdd(a.atomics, 1ull);
    }
}

template <int SRC, int MODE>
static hipError_t launch3(bool combine, const TopViewArgs &a, int batch, hipStream_t st) {
    const dim3 grid((a.W + 255) / 256, a.H, batch), block(256);
    if (combine) {
        if (a.atomics) hipLaunchKernelGGL((k_top_view<SRC, MODE, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_top_view<SRC, MODE, true, false>), grid, block, 0, st, a);
    } else {
        if (a.atomics) hipLaunchKernelGGL((k_top_view<SRC, MODE, false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_top_view<SRC, MODE, false, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

template <int SRC>
static hipError_t launch2(int mode, bool combine, const TopViewArgs &a, int batch, hipStream_t st) {
    return mode == TV_MODE_REFERENCE ? launch3<SRC, TV_MODE_REFERENCE>(combine, a, batch, st) : launch3<SRC, TV_MODE_COUNT>(combine, a, batch, st);
}

hipError_t launch_top_view(int src, int mode, bool combine, const TopViewArgs &a, int batch, hipStream_t st) {
    switch (src) {
        case TV_SRC_POINTS: return launch2<TV_SRC_POINTS>(mode, combine, a, batch, st);
        case TV_SRC_DMAP: return launch2<TV_SRC_DMAP>(mode, combine, a, batch, st);
        case TV_SRC_D1: return launch2<TV_SRC_D1>(mode, combine, a, batch, st);
    }
    return hipErrorInvalidValue;
}

// Four cells per thread: two 16-B key loads, one dword store where `out` allows it.
__global__ __launch_bounds__(256) void k_top_view_finalize(const uint64_t *__restrict__ keys, uint8_t *__restrict__ out, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 3 < n && ((reinterpret_cast<uintptr_t>(keys + i) & 15) == 0) && ((reinterpret_cast<uintptr_t>(out + i) & 3) == 0)) {
        const ulonglong2 k0 = *reinterpret_cast<const ulonglong2 *>(keys + i), k1 = *reinterpret_cast<const ulonglong2 *>(keys + i + 2);
        *reinterpret_cast<uint32_t *>(out + i) = (uint32_t)(k0.x & 0xff) | ((uint32_t)(k0.y & 0xff) << 8) | ((uint32_t)(k1.x & 0xff) << 16) | ((uint32_t)(k1.y & 0xff) << 24);
    } else {
        for (size_t c = i; c < n && c < i + 4; c++) out[c] = (uint8_t)(keys[c] & 0xff);
    }
}

hipError_t launch_top_view_finalize(const uint64_t *keys, uint8_t *out, size_t n, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_top_view_finalize, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, st, keys, out, n);
    return hipGetLastError();
}

}  // namespace sv
