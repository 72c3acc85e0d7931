// Launch interface of flow_kernels.hip (stereo visual odometry: temporal matches and the sums of one pose round: flow.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sv {

enum {
    FLOW_THREADS = 256,            // a workgroup of the match kernel: four wavefronts, a lattice point each
    FLOW_WAVES = FLOW_THREADS / 64,
    FLOW_R_MAX = 7,                // the patch is (2 r + 1)^2, at most 15 x 15: 15 rows of 4 dwords, 60 lanes' worth
    FLOW_CANDIDATES_MAX = 16384,   // a candidate's index takes 14 bits beside its cost (at most 225 * 255 < 2^16) in a 32-bit key
    FLOW_WINDOW_BYTES = 16384,     // LDS of a wavefront's window at most: 64 KB a workgroup
    FLOW_REC_WORDS = 8,            // a lattice point's record in the workspace: u0, v0, d0q (0: no match), u1, v1, d1q, best, second
    FLOW_DQ_MAX = 1 << 20,         // a disparity in 1/16 px that makes a point: 1 .. 2^20
    FLOW_CAPACITY_MAX = 65536,     // matches per frame
    FLOW_SUM_WORDS = 32,           // inside, inliers, dinliers, E, Ed, g[6], A[21]
    FLOW_SUM_THREADS = 256,        // a workgroup of the score kernel: a match per lane
    FLOW_SUM_CHUNKS_MAX = FLOW_CAPACITY_MAX / FLOW_SUM_THREADS,  // 256 partials per frame at most
    FLOW_GATE_MAX = 1 << 20,
    FLOW_J_MAX = 1 << 20
};

// dwords of a window row: the bytes of the row rounded up, one more for the dword behind a patch row's last, made odd so that the rows
// that the lanes of a wavefront read at a time start in different banks
inline int flow_pitch(int r, int wx) {
    const int p = (2 * wx + 2 * r + 1 + 3) / 4 + 1;
    return p | 1;
}
inline long long flow_window_bytes(int r, int wx, int wy) { return 4ll * flow_pitch(r, wx) * (2 * wy + 2 * r + 1); }

struct FlowCamera {
    double f, cx, cy, b16, fb, fb16;  // the host's products: b16 = 16 b, fb = f b, fb16 = f b16
};

struct FlowMatchArgs {
    const uint8_t *prev, *cur;  // [B][H][W]
    const float *d_prev;        // [B][H][W]
    const float *d_cur;         // [B][H][W] or NULL
    const double *guess;        // [B][12] or NULL: the identity, no projection
    FlowCamera cam;
    int B, H, W;
    int step, r, wx, wy, ratio, max_cost, capacity;
    int nlx, nly;        // lattice points per row and column: ceil(W / step), ceil(H / step)
    int pitch, rows;     // of a window in LDS: dwords per row, 2 wy + 2 r + 1
    int32_t *rec;        // workspace: [B][nly * nlx][FLOW_REC_WORDS]
    int32_t *matches;    // [B][capacity][6]
    int32_t *cost;       // [B][capacity][2]
    int32_t *counts;     // [B]
};

struct FlowSumsArgs {
    const int32_t *matches;  // [B][cap][6]
    const int32_t *counts;   // [B]
    const double *poses;     // [B][12]
    FlowCamera cam;
    int B, cap;
    int n_chunks;            // ceil(cap / FLOW_SUM_THREADS)
    long long gate_q, dgate_q;
    unsigned long long *partials;  // workspace: [B][n_chunks][FLOW_SUM_WORDS]
    long long *sums;               // [B][FLOW_SUM_WORDS]
};

// Two kernels: a wavefront per lattice point writes the point's record (grid (ceil(points / 4), B), dynamic LDS 4 windows), a workgroup
// per frame packs the records of the matches in point order and fills the rows behind them with -1.
hipError_t launch_flow_match(const FlowMatchArgs &a, hipStream_t st);
// Two kernels: a lane per match, a partial per chunk of 256 matches (grid (n_chunks, B); left out for cap == 0), the partials added per frame.
hipError_t launch_flow_sums(const FlowSumsArgs &a, hipStream_t st);

}  // namespace sv
