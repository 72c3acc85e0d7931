// Launch interface of track_kernels.hip (the boxes of two frames linked by their temporal matches, and each linked box's motion: track.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "flow_kernels.h"

namespace sv {

enum {
    TRACK_THREADS = 256,        // a workgroup of the votes and the sums kernel: a chunk of 256 matches of a frame, a match per lane
    TRACK_BOXES_MAX = 64,       // boxes per frame: a match's membership in the boxes of one frame is one 64-bit word
    TRACK_VOTE_PITCH = TRACK_BOXES_MAX + 1,  // a row of the votes table in LDS: 64 current boxes and the members
    TRACK_SUM_WORDS = 16,       // n, inside, ru, rv, rd, E, m[3], m^2[3], p[3], 0
    TRACK_BAND_MAX = 1 << 20,
    TRACK_GATE_MAX = 1 << 20,
    TRACK_SHARE_MAX = 256,
    TRACK_M_MAX = 1 << 20,      // |m|, |ru|, |rv|, |rd| of a match are clamped to it
    TRACK_P_MAX = 1 << 30,      // |p| of a match is clamped to it
    TRACK_STOP_MASK = 3         // flags bits 0 .. 1: the kernels left out from the end - 1 the sums, 2 the link too, 3 the votes too
};

struct TrackArgs {
    const int32_t *matches;  // [B][cap][6]
    const int32_t *counts;   // [B]
    const double *poses;     // [B][12]
    FlowCamera cam;
    const int32_t *boxes0, *boxes1;  // [B][M][4]
    const int32_t *n0, *n1;          // [B] or NULL: M each
    const int32_t *q0, *q1;          // [B][M]
    const int32_t *centre;           // [B][M][3] or NULL
    int B, cap, M, W, H;
    int n_chunks;            // ceil(cap / TRACK_THREADS)
    int min_votes, share, flags;
    long long band_q, gate_m;
    unsigned long long *words;  // workspace: [B][cap][2], a match's membership words of frame k - 1 and of frame k
    int32_t *votes;             // [B][M][M + 1]
    int32_t *link;              // [B][M][4]
    unsigned long long *sums;   // [B][M][TRACK_SUM_WORDS], int64 in two's complement
};

// Four kernels: votes and sums cleared; a lane per match - the membership words, the votes added in LDS and flushed by integer atomicAdd
// (grid (n_chunks, B); left out for cap == 0); a wavefront per frame - the link of every previous box; a lane per match - the sums of the
// linked boxes added in LDS and flushed by 64-bit integer atomicAdd.  M >= 1.
hipError_t launch_object_links(const TrackArgs &a, hipStream_t st);

}  // namespace sv
