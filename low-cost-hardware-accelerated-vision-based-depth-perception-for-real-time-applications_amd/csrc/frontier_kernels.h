// Launch interface of frontier_kernels.hip (the frontier cells and the frontier clusters of frontier.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

// A workgroup of the tile kernel owns FRONTIER_TILE^2 cells; FRONTIER_SEAM threads walk the first row and the first column of a tile.  The
// element-wise kernels give a thread FRONTIER_CHUNK consecutive cells; a workgroup of the cells kernel owns FRONTIER_SPAN of them and
// stages the rows above and below as well where a row has at most FRONTIER_HALO_COLS cells.  An index fits FRONTIER_INDEX_BITS bits.
enum { FRONTIER_THREADS = 256, FRONTIER_TILE = 64, FRONTIER_SEAM = 2 * FRONTIER_TILE, FRONTIER_CHUNK = 16, FRONTIER_SPAN = 8192, FRONTIER_HALO_COLS = 4096,
       FRONTIER_BLOCKED = 255, FRONTIER_CELLS_MAX = 8000000, FRONTIER_INDEX_BITS = 23, FRONTIER_CAPACITY_MAX = 65535 };

// What sv_debug_frontier fixes: the tile phase and the seams, or every member its own parent and all links through the global union.
enum { FRONTIER_TILES = 0, FRONTIER_NO_TILES = 1 };

struct FrontierCellsArgs {
    const int16_t *logodds;    // [rows][cols]
    const int32_t *last_seen;  // [rows][cols]
    const uint8_t *pen;        // [rows][cols] or NULL
    uint8_t *mask;             // [rows][cols]
    int rows, cols, occupied, free_;
};

struct FrontierArgs {
    const uint8_t *mask;           // [rows][cols]
    int32_t *label;                // [rows][cols]
    int32_t *clusters;             // [capacity][8], -1 everywhere before the kernels
    long long *sums;               // [capacity][2], 0 everywhere before the kernels
    int32_t *info;                 // [4]
    int32_t *size;                 // workspace [cells], 0 before the kernels: a root's member count, then its rank or -1
    unsigned long long *key;       // workspace [capacity], all ones before the kernels: d2 << 23 | index of the representative so far
    int32_t *parent;               // workspace [cells]
    int32_t *blocks;               // workspace [n_blocks][4]: kept roots, roots, members of a block of FRONTIER_THREADS * FRONTIER_CHUNK cells; then the rank of its first kept root
    unsigned long long *counters;  // debug: fetch_mins on global memory, tiles with a member; or NULL
    int rows, cols, tiles_x, tiles_y, n_blocks, min_cells, capacity, no_tiles;
};

hipError_t launch_frontier_cells(const FrontierCellsArgs &a, hipStream_t st);
// The whole call on `st`: the four memsets and the kernels from the tiles to the representatives.  size_bytes and key_bytes are the
// spans of the two workspace blocks that the memsets fill.
hipError_t launch_frontier_clusters(const FrontierArgs &a, size_t size_bytes, size_t key_bytes, hipStream_t st);

}  // namespace sv
