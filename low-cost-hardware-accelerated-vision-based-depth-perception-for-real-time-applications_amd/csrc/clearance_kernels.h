// Launch interface of clearance_kernels.hip (the clearance field and the path check of clearance.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_map_cells.h"

namespace sv {

// A column-pass lane owns CLEARANCE_STRIP rows of one column (their source flags are one 64-bit word); a row-pass workgroup owns
// CLEARANCE_TILE_ROWS rows x CLEARANCE_THREADS columns and stages them with a halo of R columns on both sides; the fused kernel owns
// CLEARANCE_FUSED_TILE^2 cells with a halo of R <= CLEARANCE_FUSED_MAX_R all round.  A path check has at most CLEARANCE_MAX_DISCS discs.
enum { CLEARANCE_THREADS = 256, CLEARANCE_STRIP = 64, CLEARANCE_TILE_ROWS = 8, CLEARANCE_MAX_R = 254, CLEARANCE_FUSED_TILE = 64, CLEARANCE_FUSED_MAX_R = 32,
       CLEARANCE_MAX_DISCS = 64, CLEARANCE_NONE = 255, CLEARANCE_FAR = 65535 };

// What sv_debug_clearance fixes: the call's own choice, both passes in one kernel (R <= CLEARANCE_FUSED_MAX_R), the two kernels, and the
// two kernels with every lane walking all 2 R + 1 taps.
enum { CLEARANCE_AUTO = 0, CLEARANCE_FUSED = 1, CLEARANCE_TWO_PASS = 2, CLEARANCE_TWO_PASS_FULL = 3 };

struct ClearanceArgs {
    const int16_t *logodds;       // [rows][cols]
    const int32_t *last_seen;     // [rows][cols], or NULL
    uint8_t *g;                   // workspace [rows][cols]: rows to the nearest source of the column, CLEARANCE_NONE beyond R
    uint16_t *d2;                 // [rows][cols]
    unsigned long long *taps;     // debug counter of the row pass's taps, or NULL
    int rows, cols, R, t_occ, unknown;
    int early_exit;               // a wavefront stops once no lane of it can still improve
};

struct ClearanceDiscs {
    double px[CLEARANCE_MAX_DISCS], py[CLEARANCE_MAX_DISCS];
    int32_t r2[CLEARANCE_MAX_DISCS];
};

struct ClearancePathsArgs {
    const uint16_t *d2;           // [rows][cols]
    const double *poses;          // [n_paths][n_steps][4] = tx, ty, c, s
    int32_t *first_hit, *min_d2, *n_outside;  // [n_paths] each
    int n_paths, n_steps, n_discs;
    MapCells m;                   // the map
};

// The field on `st`: passes & 1 the column pass, passes & 2 the row pass (3 is the call; the others are measurement aids), or - fused -
// one kernel that does both.
hipError_t launch_clearance(const ClearanceArgs &a, hipStream_t st, bool fused, int passes);
hipError_t launch_clearance_paths(const ClearancePathsArgs &a, const ClearanceDiscs &discs, hipStream_t st);

}  // namespace sv
