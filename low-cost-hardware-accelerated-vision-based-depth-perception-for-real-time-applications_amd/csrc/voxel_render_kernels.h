// Launch interface of voxel_render_kernels.hip (a voxel map rendered into a camera: voxel_render.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"  // the map's buffer: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES

namespace sv {

enum {
    VRENDER_THREADS = 256,      // a workgroup of every kernel here: four wavefronts
    VRENDER_VIEWS = 8,          // views a workgroup of the table walks draws a voxel into: the table is walked ceil(views / 8) times
    VRENDER_MAX_GROUPS = 2048,  // workgroups of a table walk at most per view group: a larger table is walked in strides
    VRENDER_R_MAX = 8,          // r_max at most: a voxel covers at most 17 x 17 pixels
    VRENDER_VIEWS_MAX = 4096,
    VRENDER_SIDE_MAX = 8192,  // width and height at most
    VRENDER_LABELS = 6
};

struct VoxelRenderArgs {
    const uint8_t *map;  // only read
    int log2_slots;      // 10 .. 27
    double lo[3], size;
    long long min_n, min_rows;  // min_n >= 1
    int since;
    double f, cx, cy, q32, q33, half_px, near, far;  // finite; f > 0, q32 != 0, half_px >= 0, 0 < near < far <= 2^20
    int width, height, r_max, views;                 // views * width * height < 2^31
    const double *cams;                              // [views][12]: R row-major, then t, world to camera
    uint32_t *depth;                                 // [views][height][width]
    unsigned long long *key;                         // [views][height][width]
    uint8_t *color;                                  // [views][height][width][4], 4-byte aligned, or NULL
    float *disparity;                                // [views][height][width], or NULL
    const float *measured;                           // [views][height][width], or NULL: then label and counts are NULL
    double tol;                                      // >= 0
    uint8_t *label;                                  // [views][height][width]
    long long *stats;                                // [views][2]: drawn, covered
    long long *counts;                               // [views][VRENDER_LABELS]
};

// Four kernels: clear (a lane per pixel), depth and key (grid (min(slots / 256, max_groups), ceil(views / VRENDER_VIEWS)), a lane per slot
// and trip), resolve (grid (ceil(height * width / 256), views), a lane per pixel).  views >= 1; max_groups in 1 .. VRENDER_MAX_GROUPS.
// stages: 0 = all four, 1 .. 3 = the first that many only (a measurement hook).
hipError_t launch_voxel_render(const VoxelRenderArgs &a, int max_groups, int stages, hipStream_t st);

}  // namespace sv
