// Launch interface of voxel_carve_kernels.hip (a voxel map carved by the sight lines of frames: voxel_carve.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"  // the map's buffer: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES, VMAP_F32 / VMAP_F64

namespace sv {

enum {
    VCARVE_THREADS = 256,      // a workgroup of every kernel here: four wavefronts
    VCARVE_STATS = 4,          // rays, steps, touched, carved
    VCARVE_MAX_GROUPS = 2048,  // workgroups of the apply kernel at most (voxel_carry_kernels.h's bound): a larger table is walked in strides
    VCARVE_REACH_MAX = 1023,   // cells a ray may span on its major axis: 2 k d + nst stays below 2^22
    VCARVE_MARGIN_MAX = 255,
    VCARVE_STEPS = 4  // steps of a ray whose table loads a lane keeps in flight together
};

struct VoxelCarveArgs {
    uint8_t *map;    // read; written by the apply kernel only, and only with `apply`
    int log2_slots;  // 10 .. 27
    double lo[3], hi[3], size;
    int nc[3];  // cells per axis, 1 .. 2^20
    const void *xyz;        // f32 or f64 [B][cap][3]
    const int32_t *weight;  // [B][cap], or NULL: every weight 1
    const int32_t *counts;  // [B]
    const double *poses;    // [B][12]: R row-major, then t
    double origin[3];       // the sensor's centre in the frame's axes, finite
    int cap;                // rows per frame
    int seq0;               // the sequence number of frame 0; seq0 + B - 1 < 2^31 - 1
    int reach, margin;      // 1 .. VCARVE_REACH_MAX, 0 .. VCARVE_MARGIN_MAX
    long long min_miss;     // >= 1
    int ratio;              // 0 .. 65535, in 1 / 256
    int apply;              // 0 or 1
    unsigned long long *miss;  // [slots], outside the map
    long long *stats;          // [VCARVE_STATS], or NULL
};

// Three kernels: zero (miss and stats cleared, the verdict of an overflowed map), rays (grid (ceil(cap / 256), batch), a lane per row;
// left out for a call without rows), apply (grid min(slots / VCARVE_THREADS, VCARVE_MAX_GROUPS), a lane per slot and trip).
hipError_t launch_voxel_carve(int dtype, const VoxelCarveArgs &a, int batch, hipStream_t st);

}  // namespace sv
