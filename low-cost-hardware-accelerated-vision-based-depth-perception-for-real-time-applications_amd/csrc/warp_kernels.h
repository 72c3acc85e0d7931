// Launch interface of warp_kernels.hip (the previous frame's disparity map warped into the current frame: warp.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_kernels.h"

namespace sv {

enum {
    WARP_THREADS = 256,     // a workgroup of every kernel: 256 consecutive pixels of a frame, lanes along u
    WARP_E_MAX = 4,         // a source covers (e + 1)^2 target pixels, e <= e_max <= 4
    WARP_PD_MAX = 1 << 20,  // a predicted disparity in 1/16 px that is kept: 1 .. 2^20
    WARP_TOL_MAX = 1 << 20,
    WARP_REL_MAX = 256,
    WARP_COUNT_WORDS = 8,   // sources kept, pixels covered, pixels per label 0 .. 5
    WARP_MODE_FILL = 0,
    WARP_MODE_CONFIRM = 1,
    WARP_MODE_REJECT = 2
};

struct WarpArgs {
    const float *d_prev;   // [B][H][W]
    const float *d_cur;    // [B][H][W] or NULL
    const double *poses;   // [B][12]
    FlowCamera cam;
    int B, H, W;
    int e_max, tol_q, rel_q, mode;
    unsigned long long *keys;  // workspace: [B][H * W], (pd << 32) | (0xffffffff - source), 0 = no source
    int32_t *expected;     // [B][H][W]
    int32_t *source;       // [B][H][W]
    uint8_t *label;        // [B][H][W], with d_cur only
    float *out;            // [B][H][W], with d_cur only
    int32_t *counts;       // [B][WARP_COUNT_WORDS]
};

// Three kernels: the keys and the counts cleared, a lane per source pixel (grid (ceil(H W / 256), B)) with one 64-bit atomicMax per
// covered pixel, a lane per target pixel that unpacks its key.
hipError_t launch_disparity_warp(const WarpArgs &a, hipStream_t st);

}  // namespace sv
