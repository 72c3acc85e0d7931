// Launch interface of occupancy_map_kernels.hip (the world map of occupancy_map.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

// A workgroup of 256 threads covers OCCMAP_TILE_ROWS x OCCMAP_TILE_COLS map cells; each of its four wavefronts covers
// OCCMAP_WAVE_ROWS x OCCMAP_TILE_COLS of them, and that strip is what the cull tests.
enum { OCCMAP_TILE_ROWS = 8, OCCMAP_TILE_COLS = 32, OCCMAP_WAVE_ROWS = 2, OCCMAP_CELL_MAX = 1 << 24 };

struct OccupancyMapArgs {
    const uint8_t *state;         // [B][frows][fcols]
    const double *poses;          // [B][4] = tx, ty, c, s
    const int16_t *logodds_in;    // [rows][cols]
    const int32_t *last_seen_in;  // [rows][cols], or NULL
    int16_t *logodds_out;
    int32_t *last_seen_out;       // NULL iff last_seen_in is
    unsigned long long *lookups;  // debug counter of the lanes that reached the `seen` test, or NULL
    int B, seq0;
    int rows, cols, top, left;
    int shift_rows, shift_cols;
    int frows, fcols;
    int l_occ, l_free, l_min, l_max;
    double half;                  // 1 / (2 scale)
    double fx0, fx1, fy0, fy1;    // the frame grid's ranges
    double fs;                    // the frame grid's scale
    double fr1, fc1;              // trunc(fx1 fs), trunc(fy1 fs) (integers)
    double reach, cell;           // half the diagonal of a wavefront's strip and one map cell, in metres
};

// Grid (ceil(cols / 32), ceil(rows / 8)), 256 threads.  cull: skip the frames a wavefront's strip cannot touch.
hipError_t launch_occupancy_fuse(const OccupancyMapArgs &a, bool cull, hipStream_t st);

}  // namespace sv
