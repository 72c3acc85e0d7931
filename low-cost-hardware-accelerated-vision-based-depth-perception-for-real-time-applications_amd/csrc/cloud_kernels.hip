// Compact coloured point clouds from disparity maps: an ordered stream compaction over a batch, fused with the reprojection (no dense
// cloud is written).  Specified in include/stereo_vision_hip.h (F), restated in stereo_vision/sv.py: compact_cloud.
//
//   visited   the pixels (x, y) with x % step == 0 && y % step == 0, numbered v = (y / step) * Wv + x / step, Wv = ceil(W / step):
//             ascending v is ascending flat index y * W + x
//   kept      candidate (DMAP: q > 0, D1: d > 0) and lo < P < hi on every axis, P from reproject.h's arithmetic; the strict comparison
//             drops inf and NaN, so a positive disparity with pos.w = 0 is not kept
//   tile      CLOUD_TILE = 1024 consecutive visited pixels, owned by ONE wavefront in both passes: four sweeps of 256, a lane taking
//             four consecutive pixels (with step 1 one 16-byte load where the frame's address allows it)
//   pass 1    k_cloud_count: tiles[b][t] = kept pixels of tile t
//   pass 2    k_cloud_scan: one workgroup per frame turns tiles[b][.] into its exclusive prefix sum and writes counts[b]
//   pass 3    k_cloud_write: the predicate again (the point is needed anyway), rank inside the sweep from four 64-bit ballots and
//             mbcnt - lanes in order, a lane's four pixels in order -, row = tiles[b][t] + kept so far in the tile + rank; rows below
//             capacity are stored
//
// The order between tiles comes from the launch boundaries alone: no workgroup waits for another one, and because a tile belongs to
// one wavefront the two big kernels need neither LDS nor a barrier.  Every load is guarded by v < n_visited, every store by
// row < capacity; a tile index is < n_tiles.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloud_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

__device__ __forceinline__ bool frame_vec_ok(const CloudArgs &a, const float *frame) {
    return a.step == 1 && (reinterpret_cast<uintptr_t>(frame) & 15) == 0;
}

template <int SRC>
__global__ __launch_bounds__(64 * CLOUD_WAVES) void k_cloud_count(CloudArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int tile = blockIdx.x * CLOUD_WAVES + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;  // the whole wavefront
    const float *frame = a.disp + (size_t)b * a.W * a.H;
    const bool vec_ok = frame_vec_ok(a, frame);
    int total = 0;
    for (int s = 0; s < CLOUD_TILE / (64 * CLOUD_QUAD); s++) {
        const uint32_t v0 = (uint32_t)tile * CLOUD_TILE + (uint32_t)(s * 64 + lane) * CLOUD_QUAD;
        int pix[CLOUD_QUAD];
        double P[CLOUD_QUAD][3];
        const unsigned keep = cloud_quad<SRC>(a, frame, vec_ok, v0, pix, P);
#pragma unroll
        for (int k = 0; k < CLOUD_QUAD; k++) total += __popcll(__ballot((keep >> k) & 1u));
    }
    if (lane == 0) a.tiles[(size_t)b * a.n_tiles + tile] = total;
}

// Exclusive prefix sum of a frame's tile counts in place: a thread owns a run of consecutive tiles.
__global__ __launch_bounds__(256) void k_cloud_scan(CloudArgs a) {
    __shared__ int s_wave[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    int32_t *t = a.tiles + (size_t)b * a.n_tiles;
    const int per = (a.n_tiles + 255) / 256;  // <= 2^13
    const int lo = tid * per < a.n_tiles ? tid * per : a.n_tiles, hi = lo + per < a.n_tiles ? lo + per : a.n_tiles;
    int own = 0;
    for (int k = lo; k < hi; k++) own += t[k];
    int total;
    int run = block_exclusive_scan<256>(own, s_wave, &total);  // every thread gets here
    for (int k = lo; k < hi; k++) {
        const int c = t[k];
        t[k] = run;
        run += c;
    }
    if (tid == 255) a.counts[b] = run;  // the last thread's run ends at the total (<= n_visited < 2^31)
}

template <int SRC, int DT>
__global__ __launch_bounds__(64 * CLOUD_WAVES) void k_cloud_write(CloudArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int tile = blockIdx.x * CLOUD_WAVES + (threadIdx.x >> 6);
    if (tile >= a.n_tiles) return;  // the whole wavefront
    int row = a.tiles[(size_t)b * a.n_tiles + tile];
    const float *frame = a.disp + (size_t)b * a.W * a.H;
    const bool vec_ok = frame_vec_ok(a, frame);
    const size_t slot = (size_t)b * a.capacity;
    for (int s = 0; s < CLOUD_TILE / (64 * CLOUD_QUAD) && row < a.capacity; s++) {  // rows only grow: nothing later is stored either
        const uint32_t v0 = (uint32_t)tile * CLOUD_TILE + (uint32_t)(s * 64 + lane) * CLOUD_QUAD;
        int pix[CLOUD_QUAD];
        double P[CLOUD_QUAD][3];
        const unsigned keep = cloud_quad<SRC>(a, frame, vec_ok, v0, pix, P);
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < CLOUD_QUAD; k++) {
            const unsigned long long m = __ballot((keep >> k) & 1u);
            before += lanes_below(m);
            total += __popcll(m);
        }
        int r = row + before;
#pragma unroll
        for (int k = 0; k < CLOUD_QUAD; k++) {
            if ((keep >> k) & 1u) {
                if (r < a.capacity) {
                    const size_t o = slot + (size_t)r;
                    if (DT == CLOUD_F32) {
                        float *p = static_cast<float *>(a.xyz) + 3 * o;
                        p[0] = (float)P[k][0], p[1] = (float)P[k][1], p[2] = (float)P[k][2];
                    } else {
                        double *p = static_cast<double *>(a.xyz) + 3 * o;
                        p[0] = P[k][0], p[1] = P[k][1], p[2] = P[k][2];
                    }
                    if (a.color_out)
                        reinterpret_cast<uint32_t *>(a.color_out)[o] = reinterpret_cast<const uint32_t *>(a.colors)[(size_t)b * a.W * a.H + pix[k]];
                    if (a.index_out) a.index_out[o] = pix[k];
                }
                r++;
            }
        }
        row += total;
    }
}

dim3 tile_grid(const CloudArgs &a, int batch) { return dim3((a.n_tiles + CLOUD_WAVES - 1) / CLOUD_WAVES, batch); }

template <int SRC>
hipError_t launch_write_dt(int dtype, const CloudArgs &a, int batch, hipStream_t st) {
    if (dtype == CLOUD_F32)
        hipLaunchKernelGGL((k_cloud_write<SRC, CLOUD_F32>), tile_grid(a, batch), dim3(64 * CLOUD_WAVES), 0, st, a);
    else if (dtype == CLOUD_F64)
        hipLaunchKernelGGL((k_cloud_write<SRC, CLOUD_F64>), tile_grid(a, batch), dim3(64 * CLOUD_WAVES), 0, st, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

hipError_t launch_cloud_count(int src, const CloudArgs &a, int batch, hipStream_t st) {
    if (src == CLOUD_SRC_DMAP)
        hipLaunchKernelGGL((k_cloud_count<CLOUD_SRC_DMAP>), tile_grid(a, batch), dim3(64 * CLOUD_WAVES), 0, st, a);
    else if (src == CLOUD_SRC_D1)
        hipLaunchKernelGGL((k_cloud_count<CLOUD_SRC_D1>), tile_grid(a, batch), dim3(64 * CLOUD_WAVES), 0, st, a);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_cloud_scan(const CloudArgs &a, int batch, hipStream_t st) {
    hipLaunchKernelGGL(k_cloud_scan, dim3(batch), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_cloud_write(int src, int dtype, const CloudArgs &a, int batch, hipStream_t st) {
    if (src == CLOUD_SRC_DMAP) return launch_write_dt<CLOUD_SRC_DMAP>(dtype, a, batch, st);
    if (src == CLOUD_SRC_D1) return launch_write_dt<CLOUD_SRC_D1>(dtype, a, batch, st);
    return hipErrorInvalidValue;
}

}  // namespace sv
