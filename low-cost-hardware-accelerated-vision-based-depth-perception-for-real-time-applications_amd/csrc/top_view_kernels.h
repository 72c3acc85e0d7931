// Launch interface of top_view_kernels.hip (the bird's-eye-view rasteriser of top_view.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reproject.h"

namespace sv {

enum TopViewSource {
    TV_SRC_POINTS = 0,  // f64 cloud [B][N][3]
    TV_SRC_DMAP = 1,    // disparity [B][H][W] -> saturate(round_half_even(4 d)) -> reproject.h (every pixel, like k_reproject_batch)
    TV_SRC_D1 = 2,      // disparity [B][H][W] -> reproject.h on the float d itself; pixels with d <= 0 are skipped
};
enum { TV_MODE_REFERENCE = 0, TV_MODE_COUNT = 1 };  // == SV_TOPVIEW_REFERENCE / SV_TOPVIEW_COUNT

struct TopViewArgs {
    ReprojectArgs rp;            // disparity sources only
    const double *points;        // TV_SRC_POINTS
    const float *disp;           // TV_SRC_DMAP / TV_SRC_D1
    void *grid;                  // uint64 [B][rows][cols] keys (reference mode) or int32 [B][rows][cols] counts
    unsigned long long *atomics; // debug counter of the grid atomics issued, or NULL
    int W, H;                    // points: W = N, H = 1
    int rows, cols;
    double x0, x1, y0, y1, z0, z1;
    double s;                    // scale
    double x1s, y1s;             // trunc(x1 * s), trunc(y1 * s) (integers)
    double max_dist;             // sqrt(x1*x1 + y1*y1), on the host
};

// Grid (ceil(W / 256), H, batch), 256 threads (points: W = N, H = 1).  combine: one atomic per run of equal cells in a wavefront.
hipError_t launch_top_view(int src, int mode, bool combine, const TopViewArgs &a, int batch, hipStream_t st);
// Reference mode: u8 grid = low byte of each key (0 for an empty cell), n cells.
hipError_t launch_top_view_finalize(const uint64_t *keys, uint8_t *out, size_t n, hipStream_t st);

}  // namespace sv
