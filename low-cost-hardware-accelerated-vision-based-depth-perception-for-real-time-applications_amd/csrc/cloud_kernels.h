// Launch interface of cloud_kernels.hip (the compact coloured point clouds of cloud.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reproject.h"

namespace sv {

enum { CLOUD_SRC_DMAP = 0, CLOUD_SRC_D1 = 1 };  // == SV_CLOUD_DMAP / SV_CLOUD_D1
enum { CLOUD_F32 = 0, CLOUD_F64 = 1 };          // == SV_CLOUD_F32 / SV_CLOUD_F64
enum {
    CLOUD_TILE = 1024,           // visited pixels per tile: the unit that is counted, scanned and written by ONE wavefront
    CLOUD_WAVES = 4,             // tiles per workgroup of 256 threads
    CLOUD_QUAD = 4,              // consecutive visited pixels per lane and sweep (one 16-byte load with step 1)
};

struct CloudArgs {
    ReprojectArgs rp;
    double lo[3], hi[3];
    const float *disp;      // [B][H][W]
    const uint8_t *colors;  // [B][H][W][4], or NULL
    void *xyz;              // [B][capacity][3] float or double
    uint8_t *color_out;     // [B][capacity][4], or NULL
    int32_t *index_out;     // [B][capacity], or NULL
    int32_t *counts;        // [B]
    int32_t *tiles;         // workspace [B][n_tiles]: the tile's count, after the scan the number of kept points before the tile
    int W, H, step, Wv;     // Wv = ceil(W / step) visited columns
    int n_visited, n_tiles; // ceil(W / step) * ceil(H / step), ceil(n_visited / CLOUD_TILE)
    int capacity;
};

// Grid (ceil(n_tiles / CLOUD_WAVES), batch), 256 threads: tiles[b][t] = kept points of tile t.
hipError_t launch_cloud_count(int src, const CloudArgs &a, int batch, hipStream_t st);
// Grid (batch), 256 threads: tiles[b][.] becomes its exclusive prefix sum, counts[b] the total.
hipError_t launch_cloud_scan(const CloudArgs &a, int batch, hipStream_t st);
// The count kernel's grid: the kept points of tile t go to rows tiles[b][t].. of frame b's slot, those below capacity are stored.
hipError_t launch_cloud_write(int src, int dtype, const CloudArgs &a, int batch, hipStream_t st);

#ifdef __HIP__  // the device code the kernels of (F) and (I) share

// The predicate of (F), shared by cloud_kernels.hip (N = CLOUD_QUAD) and voxel_kernels.hip (N = 1): a lane's N consecutive visited pixels
// v0 .. v0 + N - 1 (those < n_visited): bit k of the result = pixel k is kept; pix[k] = its flat index, P[k] = its point (read only
// where the bit is set).  vec_ok is read with N = 4 only (frame_vec_ok).
template <int SRC, int N>
__device__ __forceinline__ unsigned cloud_run(const CloudArgs &a, const float *frame, bool vec_ok, uint32_t v0, int *pix, double (*P)[3]) {
    const uint32_t n = (uint32_t)a.n_visited;
    if (v0 >= n) return 0u;
    const uint32_t vy = v0 / (uint32_t)a.Wv;
    int vx = (int)(v0 - vy * (uint32_t)a.Wv), x[N], y[N];
    int cx = vx * a.step, cy = (int)vy * a.step;  // <= W - 1, H - 1
    const int have = n - v0 < (uint32_t)N ? (int)(n - v0) : N;
#pragma unroll
    for (int k = 0; k < N; k++) {
        x[k] = cx, y[k] = cy;
        pix[k] = k < have ? cy * a.W + cx : 0;  // < W * H
        if (k + 1 < have) {                      // the next pixel exists: cx <= W - 1, cy <= H - 1 whatever the step
            if (++vx == a.Wv) vx = 0, cx = 0, cy += a.step;
            else cx += a.step;
        }
    }
    float dv[N];
    if (N == 4 && vec_ok && have == N) {  // step 1: pix[k] = v0 + k, v0 % 4 == 0
        const float4 f = *reinterpret_cast<const float4 *>(frame + v0);
        dv[0] = f.x, dv[1] = f.y, dv[2] = f.z, dv[3] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) dv[k] = k < have ? frame[pix[k]] : 0.f;  // 0 is no candidate
    }
    unsigned keep = 0u;
#pragma unroll
    for (int k = 0; k < N; k++) {
        double d;
        bool cand;
        if (SRC == CLOUD_SRC_DMAP) {
            const int q = sv_dmap_u8(dv[k]);
            cand = q > 0, d = (double)q;
        } else {
            cand = dv[k] > 0.f, d = (double)dv[k];  // NaN is no candidate
        }
        if (cand) {
            double X, Y, Z;
            sv_reproject_point(a.rp, (double)x[k], (double)y[k], d, X, Y, Z);
            if (a.lo[0] < X && X < a.hi[0] && a.lo[1] < Y && Y < a.hi[1] && a.lo[2] < Z && Z < a.hi[2]) {
                keep |= 1u << k;
                P[k][0] = X, P[k][1] = Y, P[k][2] = Z;
            }
        }
    }
    return keep;
}

template <int SRC>
__device__ __forceinline__ unsigned cloud_quad(const CloudArgs &a, const float *frame, bool vec_ok, uint32_t v0, int *pix, double (*P)[3]) {
    return cloud_run<SRC, CLOUD_QUAD>(a, frame, vec_ok, v0, pix, P);
}

#endif

}  // namespace sv
