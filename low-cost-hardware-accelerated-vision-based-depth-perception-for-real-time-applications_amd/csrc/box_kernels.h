// Launch interface of box_kernels.hip (the per-box 3-D positions of box_positions.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "reproject.h"

namespace sv {

enum BoxSource {
    BOX_SRC_POINTS = 0,  // f64 cloud [B][H][W][3]; no disparity, BOX_SEL_ALL only
    BOX_SRC_DMAP = 1,    // disparity [B][H][W]: q = saturate_u8(round_half_even(4 d)), point of (double)q; valid iff q > 0
    BOX_SRC_D1 = 2,      // disparity [B][H][W]: q = min(round_half_even(4 d), 4095), point of (double)d; valid iff d > 0
};
enum { BOX_SEL_ALL = 0, BOX_SEL_VALID = 1, BOX_SEL_NEAR = 2 };  // == SV_BOX_ALL / SV_BOX_VALID / SV_BOX_NEAR
enum { BOX_BINS = 4096 };                                      // histogram bins of q (16 KB of LDS)

struct BoxArgs {
    ReprojectArgs rp;        // disparity sources only
    const double *points;    // BOX_SRC_POINTS
    const float *disp;       // BOX_SRC_DMAP / BOX_SRC_D1
    const int32_t *boxes;    // [B][max_boxes][4] = x, y, w, h
    const int32_t *n_boxes;  // [B], or NULL = max_boxes each
    double *pos;             // [B][max_boxes][3]
    int32_t *stat;           // [B][max_boxes][4], or NULL
    int W, H, max_boxes, band;
};

// Grid (max_boxes, batch), 256 threads: one workgroup per box; a box at or beyond n_boxes[b] writes nothing.
hipError_t launch_box_positions(int src, int select, const BoxArgs &a, int batch, hipStream_t st);

}  // namespace sv
