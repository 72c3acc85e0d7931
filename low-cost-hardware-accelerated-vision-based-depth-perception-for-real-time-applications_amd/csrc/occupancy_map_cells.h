// The rules that make the flat world map one map for its readers - the match (map_match_kernels.hip), the path check
// (clearance_kernels.hip), the view (view_kernels.hip), the frontier cells (frontier_kernels.hip) - and for the voxel map's way into it
// (voxel_flatten_kernels.hip) -, written down once: the map's geometry
// words, a vehicle point's way under a pose into a cell, a cell's state, and the step of the line rule, which the per-frame grid's ray
// kernel (occupancy_kernels.hip) walks as well.  Plain inline functions and one struct; what a stage does with the cell it has found
// stays in the stage.  The definitions are include/stereo_vision_hip.h (K)'s, restated in stereo_vision/sv.py (occupancy_cells_of,
// occupancy_map_state, occupancy_ray_cells).  The way back, a cell's centre, has one user (k_occupancy_fuse) and stays there.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stereo_vision_hip.h"

namespace sv {

// Cell (r, c) of the map holds the points with floor(X ms) = top - 1 - r and floor(Y ms) = left - 1 - c.
struct MapCells {
    int rows, cols, top, left;
    double ms;                          // the map's scale
    double gx_lo, gx_hi, gy_lo, gy_hi;  // floor(X ms) and floor(Y ms) of the map's last and first row and column
};

inline MapCells map_cells_of(const sv_occupancy_map_spec &s) {
    return {s.rows, s.cols, s.top, s.left, (double)s.scale, (double)(s.top - s.rows), (double)(s.top - 1), (double)(s.left - s.cols), (double)(s.left - 1)};
}

#ifdef __HIPCC__

// The vehicle point (X, Y) under the pose (tx, ty, c, s), in the world: every product, difference and sum rounded on its own, in this
// order (the build has -ffp-contract=off).
__device__ __forceinline__ void map_world(double tx, double ty, double pc, double ps, double X, double Y, double &Xw, double &Yw) {
    Xw = (pc * X - ps * Y) + tx, Yw = (ps * X + pc * Y) + ty;
}

// A world coordinate in cells, still a double: NaN and +-inf stay what they are.
__device__ __forceinline__ double map_grid(const MapCells &m, double v) { return floor(v * m.ms); }

// The cell of (gx, gy) = map_grid of a world point; false for a point outside the map, where r and c say nothing.  The comparisons are
// made in double: NaN, inf and far-away values fail them before any conversion to integer.  The test on the integers is always true
// after them; it is kept so that no input can ever address outside the map.
__device__ __forceinline__ bool map_cell(const MapCells &m, double gx, double gy, int &r, int &c) {
    if (!(gx >= m.gx_lo && gx <= m.gx_hi && gy >= m.gy_lo && gy <= m.gy_hi)) return false;
    r = m.top - 1 - (int)gx, c = m.left - 1 - (int)gy;
    return (unsigned)r < (unsigned)m.rows && (unsigned)c < (unsigned)m.cols;
}

// The state of a cell with log-odds l that was last seen at s: 0 unknown (never seen, or between the two words), 1 free, 2 occupied.
__device__ __forceinline__ uint32_t map_state(int l, int s, int occupied, int free_) { return s >= 0 ? (l >= occupied ? 2u : l <= free_ ? 1u : 0u) : 0u; }

// The states of 16 consecutive cells as 16 bytes in w: two 16-byte loads of log-odds and four of last_seen.  Both pointers are 16-byte
// aligned and all 16 cells lie inside the map: the caller's conditions, beside which it keeps a loop of its own cell by cell.
__device__ __forceinline__ void map_state16(const int16_t *logodds, const int32_t *last_seen, int occupied, int free_, uint32_t w[4]) {
    const uint4 l0 = *reinterpret_cast<const uint4 *>(logodds), l1 = *reinterpret_cast<const uint4 *>(logodds + 8);
    const uint32_t lw[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int4 s = *reinterpret_cast<const int4 *>(last_seen + 4 * q);
        const int s4[4] = {s.x, s.y, s.z, s.w};
        w[q] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int l = (int)(int16_t)(lw[2 * q + (k >> 1)] >> (16 * (k & 1)));
            w[q] |= map_state(l, s4[k], occupied, free_) << (8 * k);
        }
    }
}

// One step of the line rule on one axis.  Step k of a line of n = max(|dr|, |dc|) steps is at a0 + floor((2 k d + n) / (2 n)); it is
// walked with the remainder rem = (2 k d + n) mod 2 n, which starts at n, takes two_d = 2 d per step and carries into the coordinate
// when it leaves 0 .. two_n - 1.  |2 d| <= 2 n, so one carry at most, and the coordinate is the floor exactly.  The step is made on
// copies and stored at the end: made on the references, the kernels' loops came out as branches where they had been selects.
template <class T>
__device__ __forceinline__ void line_step(T &rem, T &coord, T two_d, T two_n) {
    T m = rem + two_d, q = coord;
    if (m >= two_n) m -= two_n, q++;
    else if (m < 0) m += two_n, q--;
    rem = m, coord = q;
}

#endif  // __HIPCC__

}  // namespace sv
