// Launch interface of occupancy_kernels.hip (the occupancy and elevation grids of occupancy.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reproject.h"

namespace sv {

enum { OCC_H_MAX = 65535, OCC_CELL_MAX = 1 << 24 };  // the largest height step; |trunc(X s)| of a sight line's end stays below the other

struct OccupancyArgs {
    ReprojectArgs rp;
    const float *disp;            // [B][H][W]
    const uint8_t *labels;        // [B][H][W]
    const int32_t *free_row;      // [B][W]
    const float *free_disp;       // [B][W]
    int32_t *cells;               // [B][rows][cols][4] = n_ground, n_obstacle, h_lo, h_hi
    int32_t *n_rays;              // [B][rows][cols]
    uint8_t *state;               // [B][rows][cols], or NULL
    unsigned long long *atomics;  // debug counter of the evidence atomics issued, or NULL
    int W, H;
    int rows, cols;
    double x0, x1, y0, y1, z0, z1;
    double s, zs;                 // scale, z_scale
    double x1s, y1s;              // trunc(x1 * s), trunc(y1 * s) (integers)
    long long r0, c0;             // the cell of the sight lines' origin; may lie outside the grid
    int min_obstacle, min_ground, min_rays;
};

// Grid (ceil(rows * cols / 256), batch), 256 threads: counts 0, h_lo INT_MAX, h_hi -1 (one 16-byte store per cell), n_rays 0.
hipError_t launch_occupancy_clear(const OccupancyArgs &a, int batch, hipStream_t st);
// Grid (ceil(W / 256), H, batch), 256 threads.  combine: one set of atomics per run of equal cells in a wavefront.
hipError_t launch_occupancy_evidence(const OccupancyArgs &a, int batch, bool combine, hipStream_t st);
// Grid (ceil(W / 64), batch), 64 threads: a lane per image column.
hipError_t launch_occupancy_rays(const OccupancyArgs &a, int batch, hipStream_t st);
// Grid as clear: h_lo of empty cells becomes -1, state is written if asked for.
hipError_t launch_occupancy_finalize(const OccupancyArgs &a, int batch, hipStream_t st);

}  // namespace sv
