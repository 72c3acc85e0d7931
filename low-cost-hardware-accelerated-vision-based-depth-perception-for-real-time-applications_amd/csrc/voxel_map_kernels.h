// Launch interface of voxel_map_kernels.hip (the world-fixed voxel map of voxel_map.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

enum {
    VMAP_ENTRY_WORDS = 11,  // 64-bit words of a table entry (88 bytes): key | n | S[3] | C[4] | m | first_seq (low half), last_seq (high half)
    VMAP_HEAD_BYTES = 32,   // in front of the table: uint32 claimed, uint32 overflowed, uint64 dropped, two spare words
    VMAP_TILE = 256,        // slots of a tile of the read-out: one wavefront, four sweeps
    VMAP_WAVES = 4,         // wavefronts of a workgroup of the insert and the read-out kernels
    VMAP_F32 = 0,
    VMAP_F64 = 1
};

// The map's buffer: the head, the table (slots entries), the tiles of the read-out (int32 [slots / VMAP_TILE]).  slots is a power of two
// >= 1024, so all three are multiples of 16 bytes.
struct VoxelMapArgs {
    uint8_t *map;
    int log2_slots;  // 10 .. 27
    int capacity;    // voxels the map may hold, 1 .. 2^26
    double lo[3], hi[3], size;
    int nc[3];       // cells per axis, 1 .. 2^20
    // insert
    const void *xyz;        // f32 or f64 [B][cap][3]
    const uint8_t *color;   // [B][cap][4], 4-byte aligned, or NULL
    const int32_t *weight;  // [B][cap], or NULL: every weight 1
    const int32_t *counts;  // [B]
    const double *poses;    // [B][12]: R row-major, then t
    int cap;                // rows per frame
    int seq0;               // the sequence number of frame 0; seq0 + B - 1 < 2^31 - 1
    unsigned long long *counters;  // debug: [0] table updates issued, [1] atomic instructions they issued; or NULL
    // rows
    long long min_n, min_rows;
    int since;
    int out_capacity;
    void *xyz_out;           // f32 or f64 [out_capacity][3]
    uint8_t *color_out;      // [out_capacity][4], or NULL
    int32_t *cell_out;       // [out_capacity][3], or NULL
    long long *n_out;        // [out_capacity], or NULL
    long long *m_out;        // [out_capacity], or NULL
    int32_t *first_out;      // [out_capacity], or NULL
    int32_t *last_out;       // [out_capacity], or NULL
    long long *key_out;      // [out_capacity]
    int32_t *count_out;      // [1]
};

__host__ __device__ inline size_t vmap_bytes(int log2_slots) {
    const size_t slots = (size_t)1 << log2_slots;
    return VMAP_HEAD_BYTES + slots * VMAP_ENTRY_WORDS * 8 + slots / VMAP_TILE * sizeof(int32_t);
}

// Grid ceil(bytes / 16 / 256): the head zero, every key empty, first_seq all ones, everything else zero.
hipError_t launch_voxel_map_clear(const VoxelMapArgs &a, hipStream_t st);
// Grid (ceil(cap / 256), batch): a lane per input row.  combine: one table update per run of equal cells in a wavefront.
hipError_t launch_voxel_map_insert(int dtype, bool combine, const VoxelMapArgs &a, int batch, hipStream_t st);
// Three kernels: the qualifying slots per tile, their exclusive prefix sum and the count, the rows in slot order.
hipError_t launch_voxel_map_rows(int dtype, const VoxelMapArgs &a, hipStream_t st);

}  // namespace sv
