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

}  // namespace sv
