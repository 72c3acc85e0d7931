// A world-fixed voxel map rendered into a camera: include/stereo_vision_hip.h (U), restated in stereo_vision/sv.py (voxel_map_render).
// The map's buffer is voxel_map_kernels.h's and is only read; the filters, the centre, the read-only probe and the head are
// voxel_map_table.h's.  Four kernels in stream order; workgroups exchange data across the launch boundaries only:
//
//   clear    a lane per pixel of all views: the depth word and the key word to all ones - which read as -1, the value of a pixel without
//            a winner -; the first `views` lanes clear their view's stats (drawn = -1 for an overflowed map) and counts.
//   depth    grid (workgroups of the walk, view group).  A strided walk of the table, a lane per slot and trip: the key, then n, m and
//            last_seq for the filters - a word only where the ones before it passed -, then the three offset sums and the centre, once.
//            Then the views of the workgroup's group, VRENDER_VIEWS at most: the twelve pose words of a view are read from the same
//            address by every lane, the projection is (U)'s in double and in its order, and every pixel of the clipped square gets an
//            atomic minimum of zq on its 32-bit depth word.  `drawn` counts by ballots into registers, a counter per view of the group,
//            and leaves the workgroup as one add per view.
//   key      the same walk and the same arithmetic; where a covered pixel's depth equals the lane's zq, an atomic minimum of the key on
//            the pixel's 64-bit key word: the winner is the smallest zq, then the smallest key, whatever slot either lies in.
//   resolve  grid (pixel tile, view), a lane per pixel: the winner's colour through the read-only probe of its key, the disparity from
//            zq, the label against the measured pixel.  `covered` and the counts per label go by ballots, summed per workgroup in LDS:
//            one add per counter that is not zero.
// Atomics are integer minima and adds only, so the result is the same bits whatever the schedule.
//
// Bounds: a slot index is < slots (the walk) or masked by slots - 1 (the probe); a view index is < views; a square is clipped to 0 ..
// width - 1 by 0 .. height - 1 before any pixel is touched, and |px|, |py| < 2^30 + 1, so px +- r stays an int; a pixel index is
// < views * height * width < 2^31; the resolve kernel's lanes beyond height * width load and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_table.h"
#include "voxel_render_kernels.h"

namespace sv {

namespace {

constexpr uint32_t VRENDER_NONE = ~0u;  // the depth word of a pixel without a winner: zq < 2^28

__global__ __launch_bounds__(VRENDER_THREADS) void k_vrender_clear(VoxelRenderArgs a) {
    const size_t pixels = (size_t)a.views * a.height * a.width;  // >= views
    const size_t i = (size_t)blockIdx.x * VRENDER_THREADS + threadIdx.x;
    if (i >= pixels) return;
    a.depth[i] = VRENDER_NONE;
    a.key[i] = VMAP_EMPTY;
    if (i < (size_t)a.views) {
        a.stats[2 * i] = vmap_overflowed_before(a.map) ? -1ll : 0ll;
        a.stats[2 * i + 1] = 0ll;
        if (a.counts) {
            for (int k = 0; k < VRENDER_LABELS; k++) a.counts[VRENDER_LABELS * i + k] = 0ll;
        }
    }
}

// The pixels a voxel at Pw covers under the view `cam`, and its zq; false where it covers none.
struct Square {
    int x0, x1, y0, y1;
    uint32_t zq;
};

__device__ __forceinline__ bool vrender_square(const VoxelRenderArgs &a, const double *cam, const double *Pw, Square &s) {
    double Pc[3];
#pragma unroll
    for (int k = 0; k < 3; k++) Pc[k] = ((cam[3 * k] * Pw[0] + cam[3 * k + 1] * Pw[1]) + cam[3 * k + 2] * Pw[2]) + cam[9 + k];
    const double tz = Pc[2] / a.size;
    if (!(a.near <= tz && tz < a.far)) return false;  // NaN never passes; behind this Pc[2] > 0
    s.zq = (uint32_t)(int)(tz * 256.0);               // < 2^28
    const double u = (a.f * Pc[0]) / Pc[2] + a.cx, v = (a.f * Pc[1]) / Pc[2] + a.cy;
    const double lim = 1073741824.0;
    if (!(-lim < u && u < lim && -lim < v && v < lim)) return false;
    const int px = (int)floor(u + 0.5), py = (int)floor(v + 0.5);
    const double q = a.half_px / tz;  // >= 0, maybe inf
    const int r = q >= (double)a.r_max ? a.r_max : (int)q;
    s.x0 = px - r > 0 ? px - r : 0, s.x1 = px + r < a.width - 1 ? px + r : a.width - 1;
    s.y0 = py - r > 0 ? py - r : 0, s.y1 = py + r < a.height - 1 ? py + r : a.height - 1;
    return s.x0 <= s.x1 && s.y0 <= s.y1;
}

// PASS 0: the depth pass; PASS 1: the key pass.
template <int PASS>
__global__ __launch_bounds__(VRENDER_THREADS) void k_vrender_walk(VoxelRenderArgs a) {
    __shared__ uint32_t s_drawn[VRENDER_THREADS / 64][VRENDER_VIEWS];
    if (vmap_overflowed_before(a.map)) return;  // the whole grid
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int v0 = (int)blockIdx.y * VRENDER_VIEWS;                                  // < views
    const int nv = a.views - v0 < VRENDER_VIEWS ? a.views - v0 : VRENDER_VIEWS;  // views of this workgroup, >= 1
    const unsigned long long *table = vmap_table(a.map);
    const size_t slots = (size_t)1 << a.log2_slots;  // a multiple of VRENDER_THREADS
    const size_t image = (size_t)a.height * a.width;
    uint32_t n_drawn[VRENDER_VIEWS];  // of this wavefront, over its trips: at most slots <= 2^27 each
#pragma unroll
    for (int j = 0; j < VRENDER_VIEWS; j++) n_drawn[j] = 0;
    for (size_t slot = (size_t)blockIdx.x * VRENDER_THREADS + threadIdx.x; slot < slots; slot += (size_t)gridDim.x * VRENDER_THREADS) {  // the same trips for a workgroup
        const unsigned long long *e = table + slot * VMAP_ENTRY_WORDS;
        const unsigned long long key = e[VMAP_KEY];
        const bool live = key != VMAP_EMPTY && vmap_passes(a, e);
        double Pw[3] = {0.0, 0.0, 0.0};
        if (live) {
            const unsigned long long n = e[VMAP_N];  // >= min_n >= 1
#pragma unroll
            for (int k = 0; k < 3; k++) Pw[k] = vmap_centre(a.lo[k], a.size, key, k, e[VMAP_S + k], n);
        }
        if (!__ballot(live)) continue;  // the whole wavefront: no voxel on this trip
#pragma unroll
        for (int j = 0; j < VRENDER_VIEWS; j++) {
            if (j < nv) {  // the same for the workgroup
                Square s;
                const bool hit = live && vrender_square(a, a.cams + (size_t)(v0 + j) * 12, Pw, s);  // the same address in every lane
                if (PASS == 0) n_drawn[j] += (uint32_t)__popcll(__ballot(hit));  // every lane of the wavefront gets here
                if (hit) {
                    const size_t base = (size_t)(v0 + j) * image;
                    for (int y = s.y0; y <= s.y1; y++) {
                        for (int x = s.x0; x <= s.x1; x++) {
                            const size_t pix = base + (size_t)y * a.width + (size_t)x;
                            if (PASS == 0) atomicMin(a.depth + pix, s.zq);
                            else if (a.depth[pix] == s.zq) atomicMin(a.key + pix, key);
                        }
                    }
                }
            }
        }
    }
    if (PASS != 0) return;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < VRENDER_VIEWS; j++) s_drawn[wave][j] = n_drawn[j];
    }
    __syncthreads();  // every thread of the workgroup gets here
    if ((int)threadIdx.x >= nv) return;
    uint32_t total = 0;
    for (int w = 0; w < VRENDER_THREADS / 64; w++) total += s_drawn[w][threadIdx.x];
    if (total) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + 2 * (size_t)(v0 + (int)threadIdx.x), (unsigned long long)total);
}

__global__ __launch_bounds__(VRENDER_THREADS) void k_vrender_resolve(VoxelRenderArgs a) {
    __shared__ uint32_t s_count[VRENDER_THREADS / 64][1 + VRENDER_LABELS];  // covered, then the labels
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, v = (int)blockIdx.y;
    const size_t image = (size_t)a.height * a.width, p = (size_t)blockIdx.x * VRENDER_THREADS + threadIdx.x;
    const bool inside = p < image;
    const size_t pix = (size_t)v * image + (inside ? p : 0);
    const uint32_t zq = inside ? a.depth[pix] : VRENDER_NONE;
    const bool has = zq != VRENDER_NONE;
    int lab = -1;
    if (inside) {
        double e = 0.0;
        if (has) {
            const double z = (((double)zq + 0.5) / 256.0) * a.size;
            e = (a.f / z - a.q33) / a.q32;
        }
        if (a.color) {
            uint32_t c = 0;
            if (has) {
                const unsigned long long *table = vmap_table(a.map);
                const long long at = vmap_find(table, a.log2_slots, a.key[pix]);  // the winner's: the map holds it
                if (at >= 0) {
                    const unsigned long long *w = table + (size_t)at * VMAP_ENTRY_WORDS;
                    const unsigned long long n = w[VMAP_N];  // >= 1: it passed the filters
#pragma unroll
                    for (int j = 0; j < 4; j++) c |= (uint32_t)((2ull * w[VMAP_C + j] + n) / (2ull * n)) << (8 * j);  // <= 255
                }
            }
            reinterpret_cast<uint32_t *>(a.color)[pix] = c;
        }
        if (a.disparity) a.disparity[pix] = has ? (float)e : -1.0f;
        if (a.label) {
            const float m = a.measured[pix];
            const bool valid = __builtin_isfinite(m) && m > 0.0f;
            if (!valid || !has) {
                lab = (valid ? 1 : 0) + (has ? 2 : 0);
            } else {
                const double diff = (double)m - e;
                lab = diff > a.tol ? 4 : (diff < -a.tol ? 5 : 3);
            }
            a.label[pix] = (uint8_t)lab;
        }
    }
    // every lane of the workgroup gets here
    const uint32_t n_covered = (uint32_t)__popcll(__ballot(has));
    if (lane == 0) s_count[wave][0] = n_covered;
#pragma unroll
    for (int k = 0; k < VRENDER_LABELS; k++) {
        const uint32_t n_lab = (uint32_t)__popcll(__ballot(lab == k));
        if (lane == 0) s_count[wave][1 + k] = n_lab;
    }
    __syncthreads();
    const int k = (int)threadIdx.x;
    if (k >= 1 + VRENDER_LABELS || (k >= 1 && !a.counts)) return;
    uint32_t total = 0;
    for (int w = 0; w < VRENDER_THREADS / 64; w++) total += s_count[w][k];
    if (!total) return;
    long long *to = k == 0 ? a.stats + 2 * (size_t)v + 1 : a.counts + (size_t)VRENDER_LABELS * v + (k - 1);
    atomicAdd(reinterpret_cast<unsigned long long *>(to), (unsigned long long)total);
}

}  // namespace

hipError_t launch_voxel_render(const VoxelRenderArgs &a, int max_groups, int stages, hipStream_t st) {
    if (a.views < 1 || max_groups < 1 || max_groups > VRENDER_MAX_GROUPS) return hipErrorInvalidValue;
    const size_t image = (size_t)a.height * a.width, pixels = (size_t)a.views * image;  // < 2^31
    hipLaunchKernelGGL(k_vrender_clear, dim3((unsigned)((pixels + VRENDER_THREADS - 1) / VRENDER_THREADS)), dim3(VRENDER_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (stages == 1) return hipSuccess;
    const size_t tiles = ((size_t)1 << a.log2_slots) / VRENDER_THREADS;  // slots is a multiple of 1024
    const dim3 walk((unsigned)(tiles < (size_t)max_groups ? tiles : (size_t)max_groups), (unsigned)((a.views + VRENDER_VIEWS - 1) / VRENDER_VIEWS));
    hipLaunchKernelGGL(k_vrender_walk<0>, walk, dim3(VRENDER_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (stages == 2) return hipSuccess;
    hipLaunchKernelGGL(k_vrender_walk<1>, walk, dim3(VRENDER_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (stages == 3) return hipSuccess;
    hipLaunchKernelGGL(k_vrender_resolve, dim3((unsigned)((image + VRENDER_THREADS - 1) / VRENDER_THREADS), (unsigned)a.views), dim3(VRENDER_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
