// Launch interface of voxel_align_kernels.hip (a frame aligned to the voxel map, the sums of one ICP round: voxel_align.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"  // the map's buffer: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES, vmap_bytes

namespace sv {

enum {
    VALIGN_THREADS = 256,      // a workgroup of the score kernel: four wavefronts
    VALIGN_ROWS = 1,           // rows of a chunk a lane walks, its sums in registers: a row is a long chain of trips to memory, so a short
                               // frame is spread over as many workgroups as it has rows for (measured with 4, 2 and 1: DESIGN.md 4x)
    VALIGN_CHUNK = VALIGN_THREADS * VALIGN_ROWS,  // rows of a frame a workgroup takes at a time: 256
    VALIGN_MAX_CHUNKS = 512,   // row chunks per frame at most; with more a workgroup takes several, n_chunks apart, so the partials stay bounded
    VALIGN_WORDS = 19,         // 64-bit words of a frame's sums and of a partial: inside, pairs, W, D, P[3], Q[3], H[9]
    VALIGN_SUM_THREADS = 256,  // a workgroup of the sum kernel
    VALIGN_SUM_GROUPS = VALIGN_SUM_THREADS / VALIGN_WORDS,  // groups of 19 threads in it, a thread per word: 13
    VALIGN_D2_MAX = 3 * 511 * 511,  // the largest d2 between a row and a voxel of its 27 cells: 783363
    VALIGN_NO_SKIP = 1         // flags: look into every one of the 27 cells (sv_debug_voxel_align)
};

struct VoxelAlignArgs {
    const uint8_t *map;  // read only
    int log2_slots;      // 10 .. 27
    double lo[3], hi[3], size;
    int nc[3];           // cells per axis, 1 .. 2^20
    const void *xyz;        // f32 or f64 [B][cap][3]
    const int32_t *weight;  // [B][cap], or NULL: every weight 1
    const int32_t *counts;  // [B]
    const double *poses;    // [B][12]: R row-major, then t
    const int32_t *origin;  // [B][3]: 1/256 of a cell from lo
    int cap, B;
    int n_chunks;  // row chunks per frame: min(ceil(cap / VALIGN_CHUNK), the most there may be), at least 1
    int max_d2;    // 0 .. VALIGN_D2_MAX
    int flags;
    long long min_n, min_rows;  // min_n >= 1 here: a tombstone is no partner
    int since;
    unsigned long long *partials;  // workspace: [B][n_chunks][VALIGN_WORDS]
    long long *sums;               // [B][VALIGN_WORDS]
    long long *pair_key;           // [B][cap], or NULL with pair_d2
    int32_t *pair_d2;              // [B][cap]
};

// Two kernels: the pairs and their sums as a partial per row chunk (grid (n_chunks, B); left out for cap == 0), the partials added per
// frame (grid B).
hipError_t launch_voxel_align(int dtype, const VoxelAlignArgs &a, hipStream_t st);

}  // namespace sv
