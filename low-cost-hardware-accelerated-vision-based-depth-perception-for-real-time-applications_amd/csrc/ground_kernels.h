// Launch interface of ground_kernels.hip (the ground plane, obstacle labels and free space of ground.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

enum {
    GROUND_BINS_MAX = 4096,  // bins of one v-disparity row: 16 KB of LDS
    GROUND_STRIP = 8,        // rows per workgroup of the histogram kernel
    GROUND_THREADS = 256,    // histogram, search and pick kernels
    GROUND_COLUMNS = 64,     // columns per workgroup (one wavefront) of the label kernel
};

struct GroundArgs {
    const float *disp;    // [B][H][W]
    uint32_t *vdisp;      // [B][H][n_bins], or NULL
    int32_t *ground;      // [B][4] = vh, qb, S, n_valid
    uint8_t *labels;      // [B][H][W], or NULL
    int32_t *free_row;    // [B][W], or NULL
    float *free_disp;     // [B][W], or NULL
    uint64_t *keys;       // workspace [B][n_vh]: per horizon row the best (S << 32) | ~candidate index
    uint32_t *prefix;     // workspace [B][H][n_bins + 1]: prefix[v][j] = sum of vdisp[v][0 .. j - 1]
    int W, H, n_bins;
    int vh_lo, vh_step, n_vh;  // horizon rows vh_lo + i vh_step, i < n_vh
    int qb_step, n_qb;         // bottom-row bins (i + 1) qb_step, i < n_qb
    int tol, g_tol, min_run, min_support;
};

// Grid (ceil(H / GROUND_STRIP), batch): the histogram rows (if vdisp) and their prefix sums.  aggregate: one LDS atomic per run of
// equal bins in a wavefront instead of one per pixel (the same counts either way).
hipError_t launch_ground_hist(const GroundArgs &a, int batch, bool aggregate, hipStream_t st);
// Grid (n_vh, batch): keys[b][i] = the best candidate of horizon row i.
hipError_t launch_ground_search(const GroundArgs &a, int batch, hipStream_t st);
// Grid (batch): ground[b] from keys[b][.] and the row totals.
hipError_t launch_ground_pick(const GroundArgs &a, int batch, hipStream_t st);
// Grid (ceil(W / GROUND_COLUMNS), batch): labels, free_row and free_disp (those that are not NULL) from disp and ground.
hipError_t launch_ground_label(const GroundArgs &a, int batch, hipStream_t st);

}  // namespace sv
