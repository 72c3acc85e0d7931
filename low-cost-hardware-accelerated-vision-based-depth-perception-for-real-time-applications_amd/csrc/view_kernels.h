// Launch interface of view_kernels.hip (the expected view of the world map from candidate poses, view.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_map_cells.h"

namespace sv {

// A workgroup of VIEW_THREADS threads walks the rays of one candidate; the state kernel gives a thread VIEW_CHUNK consecutive cells.  A
// ray takes at most VIEW_REACH_MAX steps, so the window of cells a candidate can see is at most 2 * 254 + 1 = 509 cells a side: 509 rows
// of VIEW_ROW_WORDS_MAX 32-bit words in LDS.
enum { VIEW_THREADS = 256, VIEW_CHUNK = 16, VIEW_REACH_MAX = 254, VIEW_RAYS_MAX = 1024, VIEW_POSES_MAX = 65535, VIEW_ROW_WORDS_MAX = 16 };

// The status of a ray: how far it got.
enum { VIEW_FULL = 0, VIEW_HIT = 1, VIEW_EDGE = 2, VIEW_CORNER = 3, VIEW_UNKNOWN = 4, VIEW_INVALID = 5 };

// What sv_debug_view fixes: the LDS window sized by the call's reach, or always 509 cells a side.
enum { VIEW_WINDOW_BY_REACH = 0, VIEW_WINDOW_FULL = 1 };

struct ViewArgs {
    const int16_t *logodds;    // [rows][cols]
    const int32_t *last_seen;  // [rows][cols]
    uint8_t *state;            // workspace [rows][cols]: the state of every cell, written by the first kernel
    int32_t *score;            // workspace [K]: counts[.., 0], or -1 for an invalid candidate
    const double *poses;       // [K][4] = (tx, ty, c, s), K = G * P
    const double *ends;        // [n_rays][2], vehicle axes, metres
    int32_t *counts;           // [K][3]
    int16_t *end_cells;        // [K][n_rays][2]
    uint8_t *status;           // [K][n_rays]
    int32_t *best, *best_score;  // [G]
    MapCells m;                // the map
    int G, P, n_rays, reach, window, occupied, free_, max_unknown;  // window: the reach the LDS bitmap is laid out for, >= reach
};

// The whole call on `st`: the state plane, the walk of K = G * P candidates, the best of each group.  stages: 1 the state plane alone, 2
// without the best (tools/view_time.py times them apart).
hipError_t launch_view(const ViewArgs &a, hipStream_t st, int stages);

}  // namespace sv
