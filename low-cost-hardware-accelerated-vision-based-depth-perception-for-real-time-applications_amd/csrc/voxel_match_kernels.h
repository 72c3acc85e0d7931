// Launch interface of voxel_match_kernels.hip (a frame matched against the voxel map: voxel_match.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"  // the map's buffer: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES, vmap_bytes

namespace sv {

enum {
    VMATCH_THREADS = 256,      // a workgroup of every kernel here: four wavefronts
    VMATCH_ROWS = 4,           // rows of a frame a lane of the score kernel holds in registers
    VMATCH_TILE = VMATCH_THREADS * VMATCH_ROWS,  // rows of a frame a workgroup scores at a time: 1024
    VMATCH_MAX_CHUNKS = 64,    // row chunks per frame at most; with more tiles than that a workgroup takes several, VMATCH_MAX_CHUNKS apart
    VMATCH_MAX_LOG_GROUP = 6,  // a workgroup scores at most 64 candidates
    VMATCH_PLANES = 3,         // 64-bit words of a partial: inside | hits << 32, weight, d2
    VMATCH_GROUPS = 256        // candidates per workgroup of the sum kernel, and at most so many group bests per frame (P <= 65535)
};

// The best candidate of a group of the sum kernel.
struct VoxelMatchBest {
    long long weight, d2;
    int32_t index, pad;
};

struct VoxelMatchArgs {
    const uint8_t *map;  // read only
    int log2_slots;      // 10 .. 27
    double lo[3], hi[3], size;
    int nc[3];           // cells per axis, 1 .. 2^20
    const void *xyz;        // f32 or f64 [B][cap][3]
    const int32_t *weight;  // [B][cap], or NULL: every weight 1
    const int32_t *counts;  // [B]
    const double *poses;    // [B][P][12]: R row-major, then t
    int cap, B, P;
    int n_chunks;   // row chunks per frame: min(ceil(cap / VMATCH_TILE), VMATCH_MAX_CHUNKS), at least 1
    int log_group;  // a workgroup of the score kernel owns 1 << log_group candidates
    long long min_n, min_rows;
    int since;
    unsigned long long *partials;  // workspace: [B][n_chunks][VMATCH_PLANES][P]
    VoxelMatchBest *bests;         // workspace: [B][VMATCH_GROUPS]
    int32_t *inside, *hits;        // [B][P], or all four NULL
    long long *weight_out, *d2;    // [B][P]
    int32_t *best;                 // [B]
    long long *best_weight, *best_d2;
};

// Three kernels: the scores as partials per row chunk (grid (n_chunks, ceil(P / group), B); left out for cap == 0), their sums per
// candidate with the best of every 256 (grid (ceil(P / 256), B)), the best per frame (grid B).
hipError_t launch_voxel_match(int dtype, const VoxelMatchArgs &a, hipStream_t st);

}  // namespace sv
