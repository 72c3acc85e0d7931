// Launch interface of voxel_kernels.hip (the voxel-grid downsampled clouds of voxel.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloud_kernels.h"

namespace sv {

enum {
    VOXEL_ENTRY_WORDS = 9,   // 64-bit words of a table entry: key | first (low half), n (high half) | S[3] | C[4]
    VOXEL_HEAD_BYTES = 16,   // per pair behind its table: uint32 claimed slots, uint32 overflowed, two spare words
    VOXEL_MIN_CAPACITY = 512 // the table is never smaller than for this capacity
};

// The workspace of pair b starts at ws + b * pair_bytes: the table (slots entries), the head, the mask (one bit per visited pixel,
// padded to 16 bytes).  All three are multiples of 16 bytes.  c.tiles ([B][n_tiles], behind the last pair) is (F)'s.
struct VoxelArgs {
    CloudArgs c;             // (F)'s arguments: the predicate reads rp, lo, hi, disp, W, H, step, Wv, n_visited; c.capacity = rows per pair
    double size;
    int nc[3];               // cells per axis, 1 .. 2^20
    int log2_slots;          // slots = 1 << log2_slots, 10 .. 32
    int n_words;             // mask words in use: ceil(n_visited / 32)
    uint8_t *ws;
    size_t pair_bytes, mask_offset;  // mask_offset = slots * 72 + VOXEL_HEAD_BYTES
    int32_t *cell_out;       // [B][capacity][3], or NULL
    int32_t *n_out;          // [B][capacity], or NULL
    int32_t *first_out;      // [B][capacity], or NULL
    unsigned long long *counters;  // debug: [0] table updates issued, [1] atomic instructions issued; or NULL
};

// Grid (ceil(pair_bytes / 16 / 256), batch): empties the table, zeroes the head and the mask.
hipError_t launch_voxel_clear(const VoxelArgs &a, int batch, hipStream_t st);
// (F)'s tile grid: every kept point is added to its voxel's entry.  combine: one table update per run of equal cells in a wavefront.
hipError_t launch_voxel_insert(int src, bool combine, const VoxelArgs &a, int batch, hipStream_t st);
// Grid (ceil(slots / 256), batch): an occupied slot of a pair that did not overflow sets the mask bit of its first visited pixel.
hipError_t launch_voxel_mark(const VoxelArgs &a, int batch, hipStream_t st);
// Grid (ceil(n_tiles / 256), batch): tiles[b][t] = set bits of tile t's mask words (then launch_cloud_scan on a.c).
hipError_t launch_voxel_count(const VoxelArgs &a, int batch, hipStream_t st);
// (F)'s tile grid: the row of every owner pixel; counts[b] = -1 for a pair that overflowed.
hipError_t launch_voxel_write(int src, int dtype, const VoxelArgs &a, int batch, hipStream_t st);

}  // namespace sv
