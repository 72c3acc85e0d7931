// Launch interface of voxel_repose_kernels.hip (the voxels of one voxel map moved by per-frame rigid corrections into another:
// voxel_repose.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"  // the maps' buffers: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES, VMAP_TILE, vmap_bytes

namespace sv {

enum {
    VREPOSE_THREADS = 256,  // a workgroup of the table kernel: four wavefronts, a lane per source slot
    VREPOSE_STATS = 4,      // carried, filtered, outside, claimed: the carry's
    VREPOSE_MAX_GROUPS = 2048  // workgroups of the table kernel at most (voxel_carry_kernels.h's bound): a larger table is walked in strides
};

struct VoxelReposeArgs {
    uint8_t *dst;        // changed
    const uint8_t *src;  // read only; shares no byte with dst
    int dst_log2_slots, src_log2_slots;  // 10 .. 27 each
    int dst_capacity;                    // voxels dst may hold, 1 .. 2^26
    double lo[3], hi[3], size;           // dst's box and edge: what vmap_cell reads
    int nc[3];                           // cells per axis of dst, 1 .. 2^20
    double src_lo[3], src_size;          // src's: what vmap_centre reads
    const double *corr;                  // [n_corr][12], R row-major, then t
    int n_corr;                          // 1 .. 2^22
    int seq0;                            // 0 .. 2^31 - 2
    long long min_n, min_rows;           // as given: the kernel asks for n >= 1 besides
    int since;
    long long *stats;  // [VREPOSE_STATS], or NULL
};

// Two kernels: the head (one wavefront: the counts zeroed, `dropped` and the overflow flag carried over, the verdict "nothing is carried"
// left in the first word of dst's read-out scratch), then the table (grid min(slots of src / VREPOSE_THREADS, VREPOSE_MAX_GROUPS)).
hipError_t launch_voxel_repose(const VoxelReposeArgs &a, hipStream_t st);

}  // namespace sv
