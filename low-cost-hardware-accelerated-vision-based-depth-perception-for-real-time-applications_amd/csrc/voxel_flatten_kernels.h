// Launch interface of voxel_flatten_kernels.hip (a voxel map flattened into an occupancy map: voxel_flatten.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_map_cells.h"  // the flat map's geometry: MapCells
#include "voxel_map_kernels.h"    // the voxel map's buffer: VMAP_ENTRY_WORDS, VMAP_HEAD_BYTES

namespace sv {

enum {
    VFLATTEN_THREADS = 256,        // a workgroup of every kernel here: four wavefronts
    VFLATTEN_MAX_GROUPS = 2048,    // workgroups of a table walk at most: a larger table is walked in strides
    VFLATTEN_RADIUS_MAX = 8,       // the local floor's window: at most 17 x 17 flat cells
    VFLATTEN_TILE_ROWS = 16,       // the floor kernel's tile of flat cells: 16 x 64, four cells a lane,
    VFLATTEN_TILE_COLS = 64,       // with a halo of `radius` cells on every side in LDS
    VFLATTEN_CELLS_MAX = 8000000,  // rows * cols at most: COST_CELLS_MAX and FRONTIER_CELLS_MAX, the planner's
    VFLATTEN_STATS = 8,            // drawn, outside, below, ground, obstacle, overhead, occupied_cells, free_cells
    VFLATTEN_STAGES = 5            // clear, walk A, floor, walk B, resolve
};

struct VoxelFlattenArgs {
    const uint8_t *map;  // only read
    int log2_slots;      // 10 .. 27
    double lo[3], size;
    long long min_n, min_rows;  // min_n >= 1
    int since;
    MapCells m;                                  // rows * cols <= VFLATTEN_CELLS_MAX
    int l_occ, l_free, l_min, l_max;             // the flat map's: 1 .. 32767 twice, -32767 <= l_min <= 0 <= l_max <= 32767
    int mode, z_ref_q, step_q, height_q, radius;  // 0 or 1; |z_ref_q| < 2^30; 1 <= step_q < height_q < 2^28; 0 .. VFLATTEN_RADIUS_MAX
    int min_obstacle, min_ground;                // >= 1
    int16_t *logodds;                            // [rows][cols]
    int32_t *last_seen, *floor, *top;            // [rows][cols] each; last_seen holds `seen`, and in mode 1 floor (radius 0) or top (radius > 0) holds `low`, between the kernels
    int32_t *cells;                              // [rows][cols][3]
    long long *stats;                            // [VFLATTEN_STATS]
};

// Four or five kernels: clear and resolve (a lane per flat cell), walk A and walk B (min(slots / 256, max_groups) workgroups, a lane per
// slot and trip), and between the walks, in mode 1 with radius > 0, floor (a workgroup per tile of 16 x 64 flat cells).  max_groups in
// 1 .. VFLATTEN_MAX_GROUPS.  stages: 0 = all, 1 .. 4 = the first that many of the five only (a measurement hook).
hipError_t launch_voxel_flatten(const VoxelFlattenArgs &a, int max_groups, int stages, hipStream_t st);

}  // namespace sv
