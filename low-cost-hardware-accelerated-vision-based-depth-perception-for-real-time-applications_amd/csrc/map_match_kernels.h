// Launch interface of map_match_kernels.hip (the correlative match of map_match.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_map_cells.h"

namespace sv {

// MAPMATCH_CHUNK list entries are staged in LDS at a time; a compaction workgroup covers MAPMATCH_COMPACT_CELLS frame cells; a frame has at
// most MAPMATCH_PARTIALS workgroups of candidates, each of which leaves one (score, index) pair for the last kernel.
enum { MAPMATCH_THREADS = 256, MAPMATCH_CHUNK = 1024, MAPMATCH_COMPACT_ITEMS = 16, MAPMATCH_COMPACT_CELLS = MAPMATCH_THREADS * MAPMATCH_COMPACT_ITEMS,
       MAPMATCH_PARTIALS = 2048, MAPMATCH_MAX_LOG_GROUP = 8 };

// The caller's workspace: batch headers, batch x MAPMATCH_PARTIALS partial maxima, batch lists of `cap` packed cells.
struct MapMatchHeader {
    uint32_t n_occ, n_free, pad[2];  // the entries of the frame's list: the occupied ones from its front, the free ones from its back
};
struct MapMatchPartial {
    long long score;
    int32_t index, pad;
};

struct MapMatchArgs {
    const uint8_t *state;          // [B][frows][fcols]
    const double *poses;           // [B][P][4] = tx, ty, c, s
    const int16_t *logodds;        // [rows][cols]
    long long *sums;               // [B][P][2] = H, M, or NULL
    int32_t *counts;               // [B][P][2] = n_occ, n_free; NULL iff sums is
    int32_t *best;                 // [B], or NULL
    long long *best_score;         // [B]; NULL iff best is
    MapMatchHeader *headers;       // workspace
    MapMatchPartial *partials;     // workspace
    uint32_t *lists;               // workspace: [B][cap], a cell as fr | fc << 15
    unsigned long long *lookups;   // debug counter of (list entry, candidate) pairs, or NULL
    size_t cap;                    // frows * fcols
    int B, P;
    int frows, fcols;
    MapCells m;                    // the map
    int w_occ, w_free;
    int log_group, n_groups;       // a workgroup scores 1 << log_group candidates; ceil(P / that) workgroups per frame
    double hf;                     // 1 / (2 fs)
    double fr1, fc1;               // trunc(fx1 fs), trunc(fy1 fs) (integers)
};

// Three kernels on `st`: the lists (their counters cleared first), the sums and the score per candidate, the best per frame (left out
// where a.best is NULL).  stages 1 or 2 stops behind the first or the second (a measurement aid; 3 is the call).
hipError_t launch_map_match(const MapMatchArgs &a, hipStream_t st, int stages);

}  // namespace sv
