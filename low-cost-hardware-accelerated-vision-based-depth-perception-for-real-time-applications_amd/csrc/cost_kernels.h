// Launch interface of cost_kernels.hip (the penalties, the cost-to-goal field and the routes of cost.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

// A sweep's workgroup owns COST_TILE^2 cells and stages them with a one-cell halo; it relaxes them at most COST_INNER_MAX times per sweep.
// A call makes at most COST_SWEEPS_MAX sweeps, each with a word of its own to report into.  A route is walked by COST_ROUTE_LANES lanes.
enum { COST_THREADS = 256, COST_TILE = 64, COST_SIDE = COST_TILE + 2, COST_INNER_MAX = 256, COST_SWEEPS_MAX = 1024, COST_GOALS_MAX = 1024, COST_ROUTE_LANES = 8,
       COST_BLOCKED = 255, COST_PEN_MAX = 254, COST_STEP_AXIAL = 10, COST_STEP_DIAGONAL = 14, COST_CELLS_MAX = 8000000 };
constexpr int32_t COST_INF = 0x7FFFFFFF;

// What sv_debug_cost_to_goal fixes: the tiles the dirty bytes name, or every tile in every sweep.
enum { COST_DIRTY_TILES = 0, COST_ALL_TILES = 1 };

struct CostCellsArgs {
    const uint16_t *d2;  // [cells]
    uint8_t *pen;        // [cells]
    int64_t cells;
    int r2_block, soft, weight;
};

struct CostFieldArgs {
    const uint8_t *pen;            // [rows][cols]
    const int32_t *goals;          // [n_goals][2]
    int32_t *cost, *twin;          // [rows][cols] each: sweep s reads cost and writes twin where s is even, the other way where it is odd
    uint8_t *dirty[2];             // [tiles] each: sweep s reads dirty[s & 1] and writes dirty[(s + 1) & 1]
    int32_t *changed;              // [COST_SWEEPS_MAX]: word s is 1 iff sweep s of this call changed a cell
    int32_t *info;                 // [4]
    unsigned long long *counters;  // debug: tiles run, inner iterations; or NULL
    int rows, cols, tiles_x, tiles_y, n_goals, all_tiles;
};

struct CostRoutesArgs {
    const int32_t *cost;  // [rows][cols]
    const uint8_t *pen;   // [rows][cols]
    const int32_t *starts;  // [n_routes][2]
    int16_t *cells;         // [n_routes][capacity][2], -1 everywhere before the kernel
    int32_t *length, *status;  // [n_routes] each
    int rows, cols, n_routes, capacity;
};

hipError_t launch_cost_cells(const CostCellsArgs &a, hipStream_t st);
// The whole call on `st`: the memset of the sweeps' words, with init the start from the goals, `sweeps` sweeps and the kernel that writes info.
hipError_t launch_cost_to_goal(const CostFieldArgs &a, int init, int sweeps, hipStream_t st);
hipError_t launch_cost_routes(const CostRoutesArgs &a, hipStream_t st);

}  // namespace sv
