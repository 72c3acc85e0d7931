// Launch interface of voxel_carry_kernels.hip (the voxels of one voxel map carried into another: voxel_carry.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"  // the maps' buffers: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES, VMAP_TILE, vmap_bytes

namespace sv {

enum {
    VCARRY_THREADS = 256,  // a workgroup of the carry kernel: four wavefronts, a lane per source slot
    VCARRY_STATS = 4,      // carried, filtered, outside, claimed
    VCARRY_MAX_GROUPS = 2048  // workgroups of the carry kernel at most: eight wavefronts per SIMD of 256 CUs; a larger table is walked in strides
};

struct VoxelCarryArgs {
    uint8_t *dst;        // changed
    const uint8_t *src;  // read only; shares no byte with dst
    int dst_log2_slots, src_log2_slots;  // 10 .. 27 each
    int dst_capacity;                    // voxels dst may hold, 1 .. 2^26
    int dst_nc[3];                       // cells per axis of dst, 1 .. 2^20
    int shift[3];                        // whole cells added to a source cell, each in -2^20 .. 2^20
    long long min_n, min_rows;
    int since;
    long long *stats;  // [VCARRY_STATS], or NULL
};

// Two kernels: the head (one wavefront: the counts zeroed, `dropped` and the overflow flag carried over, the verdict "nothing is carried"
// left in the first word of dst's read-out scratch), then the table (grid min(slots of src / VCARRY_THREADS, VCARRY_MAX_GROUPS)).
hipError_t launch_voxel_carry(const VoxelCarryArgs &a, hipStream_t st);

}  // namespace sv
