// Launch interface of voxel_normal_kernels.hip (the voxels' surface normals and the sums of one point-to-plane round: voxel_normals.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"  // the map's buffer: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES, vmap_bytes

namespace sv {

enum {
    VNORMAL_THREADS = 256,     // a workgroup of the normals kernel: four wavefronts, a lane per slot
    VNORMAL_DIRS_MAX = 4096,   // directions of a table at most
    VNORMAL_TILE = 1024,       // directions staged in LDS at a time, eight words each: 32 KiB
    VNORMAL_NO_PRUNE = 2,      // flags: search the table for every member, also where no output needs it (sv_debug_voxel_normals)
    VPLANE_THREADS = 256,      // a workgroup of the plane score kernel
    VPLANE_CHUNK = VPLANE_THREADS,  // rows of a frame a workgroup takes at a time, a row per lane
    VPLANE_MAX_CHUNKS = 512,   // row chunks per frame at most; with more a workgroup takes several, n_chunks apart
    VPLANE_WORDS = 32,         // 64-bit words of a frame's sums and of a partial: inside, pairs, planes, W, E, g[6], A[21]
    VPLANE_SUM_THREADS = 256,  // a workgroup of the sum kernel
    VPLANE_SUM_GROUPS = VPLANE_SUM_THREADS / VPLANE_WORDS,  // groups of 32 threads in it, a thread per word: 8
    VPLANE_D2_MAX = 3 * 511 * 511,  // the largest d2 between a row and a voxel of its 27 cells
    VPLANE_LEVER_SHIFT = 4,    // the lever arm is (p - o) >> 4: 1/16 of a cell
    VPLANE_NO_SKIP = 1         // flags: look into every one of the 27 cells (sv_debug_voxel_normals)
};

struct VoxelNormalArgs {
    const uint8_t *map;  // read only
    int log2_slots;      // 10 .. 27
    int nc[3];           // cells per axis, 1 .. 2^20
    const int8_t *dirs;  // [K][4]
    int K;               // 1 .. VNORMAL_DIRS_MAX
    int min_nb, flat, wide;
    int flags;
    long long min_n, min_rows;  // min_n >= 1 here
    int since;
    int32_t *normal;     // [slots]
    long long *fit;      // [slots][4], or NULL
    unsigned long long *counts;  // [4], zeroed in front of the kernel
};

struct VoxelPlaneArgs {
    const uint8_t *map;  // read only
    int log2_slots;
    double lo[3], hi[3], size;
    int nc[3];
    const void *xyz;        // f32 or f64 [B][cap][3]
    const int32_t *weight;  // [B][cap], or NULL: every weight 1
    const int32_t *counts;  // [B]
    const double *poses;    // [B][12]
    const int32_t *origin;  // [B][3]
    const int32_t *normal;  // [slots]: a direction's index, anything else = none
    const int8_t *dirs;     // [K][4]
    int K;
    int cap, B;
    int n_chunks;
    int max_d2;
    int flags;
    long long min_n, min_rows;
    int since;
    unsigned long long *partials;  // workspace: [B][n_chunks][VPLANE_WORDS]
    long long *sums;               // [B][VPLANE_WORDS]
    long long *pair_key;           // [B][cap], or NULL with pair_d2 and pair_normal
    int32_t *pair_d2;              // [B][cap]
    int32_t *pair_normal;          // [B][cap]
};

// The counts zeroed (a memset node), then one kernel, grid slots / VNORMAL_THREADS.
hipError_t launch_voxel_normals(const VoxelNormalArgs &a, hipStream_t st);
// Two kernels: the plane pairs and their sums as a partial per row chunk (grid (n_chunks, B); left out for cap == 0), the partials added
// per frame (grid B).
hipError_t launch_voxel_plane_align(int dtype, const VoxelPlaneArgs &a, hipStream_t st);

}  // namespace sv
