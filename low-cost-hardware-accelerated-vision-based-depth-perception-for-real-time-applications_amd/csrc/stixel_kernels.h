// Launch interface of stixel_kernels.hip (the stixels and detector-free object boxes of stixels.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

enum {
    STIXEL_COLUMNS = 64,   // visited columns per workgroup (one wavefront) of the column kernel
    STIXEL_THREADS = 256,  // object kernel: visited columns per chunk
};

struct StixelArgs {
    const float *disp;      // [B][H][W]
    const uint8_t *labels;  // [B][H][W]
    int4 *stixels;          // [B][max_layers][Wv], or NULL
    int32_t *n_stixels;     // [B][Wv], or NULL
    int4 *boxes;            // [B][capacity], or NULL
    int4 *info;             // [B][capacity], or NULL
    int32_t *counts;        // [B]
    int4 *layer0;           // workspace [B][Wv]: the first stixel of each visited column, -1 without one
    int W, H, Wv;           // Wv = ceil(W / col_step) visited columns
    int n_bins, q_min, sim, max_gap, min_rows, max_layers, col_step, sim_cols, min_cols, capacity;
};

// Grid (ceil(Wv / STIXEL_COLUMNS), batch): stixels, n_stixels (those that are not NULL) and layer0 from disp and labels.
hipError_t launch_stixel_columns(const StixelArgs &a, int batch, hipStream_t st);
// Grid (batch): boxes, info (those that are not NULL) and counts from layer0.
hipError_t launch_stixel_objects(const StixelArgs &a, int batch, hipStream_t st);

}  // namespace sv
