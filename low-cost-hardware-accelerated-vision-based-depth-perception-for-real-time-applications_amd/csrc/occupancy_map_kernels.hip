// Per-frame occupancy grids fused into a world-fixed log-odds map along a trajectory: include/stereo_vision_hip.h (K), restated in
// stereo_vision/sv.py (occupancy_fuse).  One kernel, a gather:
//
//   fuse   a lane per map cell.  It reads its cell of the map coming in - at (r + shift_rows, c + shift_cols), 0 / -1 outside: the scroll -
//          keeps L and last_seen in registers over the frames b = 0 .. B - 1, and writes its cell once.  Per frame it carries its centre
//          into the frame's axes with the pose's (c, s) - two products and a sum per coordinate, no FMA (-ffp-contract=off), no
//          trigonometric function - tests it strictly against the frame grid's ranges, reads the state byte of the frame cell it fell
//          into and adds l_occ, subtracts l_free or leaves L alone, clamped.  A gather leaves no holes under rotation and needs no atomic,
//          and since a lane applies its frames in order the clamp's dependence on the order costs nothing.
//
//   tile   a workgroup covers 8 rows x 32 columns of the map, a wavefront 2 x 32 of them: wider along the columns, so that for a small
//          yaw a wavefront's state reads lie on two runs of neighbouring bytes.  The pose of frame b is one address for every lane:
//          the frame index is wave-uniform and the compiler loads the pose with scalar loads.
//
//   cull   a wavefront first tests which frames its strip can touch at all, 64 frames at a time: lane k carries the centre C of the
//          strip into the axes of frame b0 + k and compares it with the frame's ranges widened by m = reach * max(1, c^2 + s^2) + cell + e;
//          the ballot of the 64 answers is the set of frames the wavefront then applies, in order, by a loop over its set bits - a
//          wave-uniform value, so the skipped frames cost no lane anything and the test itself a 64th of a lookup per frame.  (Testing
//          one frame at a time in front of its lookups costs more than it saves: doubles have no scalar ALU, so the test occupies the
//          vector unit as long as the lookups it would skip.)
//          reach is half the strip's diagonal: every cell centre P of the strip has |P - C| <= reach, the map (dx, dy) -> (c dx + s dy,
//          c dy - s dx) scales distances by sqrt(c^2 + s^2) <= max(1, c^2 + s^2) (1 for a rotation; a (c, s) that is none is still culled
//          correctly), so in exact arithmetic |Xf(P) - Xf(C)| <= reach * that.  e = 2^-48 (|c dx| + |s dy|) at C bounds the rounding of
//          both evaluations (a few ulp of the larger product each; P's products differ from C's by at most reach, which the whole cell
//          covers), so a pose far from the map cannot cull by noise.  Outside the widened ranges no lane of the strip can be `seen`.  A
//          pose with a non-finite word fails the comparisons (NaN) or passes them (inf margin); either way no lane is seen, as without
//          the cull.
//
// No workgroup waits for another and none reads what another writes (in and out do not overlap unless the shift is zero, where each
// lane reads and writes its own cell).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_map_kernels.h"

namespace sv {

template <bool CULL, bool COUNT>
__global__ __launch_bounds__(256) void k_occupancy_fuse(OccupancyMapArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const int r0 = (int)blockIdx.y * OCCMAP_TILE_ROWS + wave * OCCMAP_WAVE_ROWS, c0 = (int)blockIdx.x * OCCMAP_TILE_COLS;
    const int r = r0 + lane / OCCMAP_TILE_COLS, c = c0 + lane % OCCMAP_TILE_COLS;
    const bool in_map = r < a.rows && c < a.cols;
    const double Xw = (double)(2 * (a.top - r) - 1) * a.half, Yw = (double)(2 * (a.left - c) - 1) * a.half;
    // the mean of the strip's first and last centre, on both axes
    const double Xc = (double)(2 * a.top - (2 * r0 + OCCMAP_WAVE_ROWS - 1) - 1) * a.half;
    const double Yc = (double)(2 * a.left - (2 * c0 + OCCMAP_TILE_COLS - 1) - 1) * a.half;

    int L = 0, seen_at = -1;
    if (in_map) {
        const long long ri = (long long)r + a.shift_rows, ci = (long long)c + a.shift_cols;
        if (ri >= 0 && ri < a.rows && ci >= 0 && ci < a.cols) {
            const size_t i = (size_t)ri * a.cols + (size_t)ci;
            L = a.logodds_in[i];
            if (a.last_seen_in) seen_at = a.last_seen_in[i];
        }
    }
    const size_t frame_cells = (size_t)a.frows * a.fcols;
    unsigned long long lookups = 0;
    // frame b into this lane's cell; b is wave-uniform, so the pose comes through scalar loads
    auto apply = [&](int b) {
        if (!in_map) return;
        const double tx = a.poses[4 * b], ty = a.poses[4 * b + 1], pc = a.poses[4 * b + 2], ps = a.poses[4 * b + 3];
        if (COUNT) lookups++;
        const double dx = Xw - tx, dy = Yw - ty;
        const double Xf = pc * dx + ps * dy, Yf = pc * dy - ps * dx;
        if (Xf > a.fx0 && Xf < a.fx1 && Yf > a.fy0 && Yf < a.fy1) {
            const int fr = (int)(a.fr1 - trunc(Xf * a.fs)), fc = (int)(a.fc1 - trunc(Yf * a.fs));
            // always true (top_view_kernels.hip's argument); kept so that no input can ever address outside the frame grid
            if ((unsigned)fr < (unsigned)a.frows && (unsigned)fc < (unsigned)a.fcols) {
                const uint32_t st = a.state[(size_t)b * frame_cells + (size_t)fr * a.fcols + fc];
                if (st == 2u) L = min(max(L + a.l_occ, a.l_min), a.l_max);
                else if (st == 1u) L = min(max(L - a.l_free, a.l_min), a.l_max);
                if (st == 1u || st == 2u) seen_at = a.seq0 + b;
            }
        }
    };
    if (CULL) {
        // 64 frames at a time: lane k tests frame b0 + k against the strip, the ballot is the set of frames to apply, in order.  Every
        // lane of the wavefront is here (none has returned), so the ballot sees all 64.
        for (int b0 = 0; b0 < a.B; b0 += 64) {
            const int b = b0 + lane;
            bool touch = false;
            if (b < a.B) {
                const double tx = a.poses[4 * b], ty = a.poses[4 * b + 1], pc = a.poses[4 * b + 2], ps = a.poses[4 * b + 3];
                const double dx = Xc - tx, dy = Yc - ty;
                const double cx = pc * dx, sy = ps * dy, cy = pc * dy, sx = ps * dx;
                const double Xf = cx + sy, Yf = cy - sx;
                const double n = pc * pc + ps * ps;
                const double m = a.reach * (n > 1.0 ? n : 1.0) + a.cell;
                const double mx = m + (fabs(cx) + fabs(sy)) * 0x1p-48, my = m + (fabs(cy) + fabs(sx)) * 0x1p-48;
                touch = Xf > a.fx0 - mx && Xf < a.fx1 + mx && Yf > a.fy0 - my && Yf < a.fy1 + my;
            }
            unsigned long long todo = __ballot(touch);
            while (todo) {  // wave-uniform: the ballot is one value for the wavefront
                const int k = __builtin_ctzll(todo);
                todo &= todo - 1;
                apply(__builtin_amdgcn_readfirstlane(b0 + k));
            }
        }
    } else {
        for (int b = 0; b < a.B; b++) apply(b);
    }
    if (in_map) {
        const size_t i = (size_t)r * a.cols + c;
        a.logodds_out[i] = (int16_t)L;
        if (a.last_seen_out) a.last_seen_out[i] = seen_at;
    }
    if (COUNT && lookups) atomicAdd(a.lookups, lookups);
}

hipError_t launch_occupancy_fuse(const OccupancyMapArgs &a, bool cull, hipStream_t st) {
    const dim3 grid((a.cols + OCCMAP_TILE_COLS - 1) / OCCMAP_TILE_COLS, (a.rows + OCCMAP_TILE_ROWS - 1) / OCCMAP_TILE_ROWS), block(256);
    if (cull) {
        if (a.lookups) hipLaunchKernelGGL((k_occupancy_fuse<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_occupancy_fuse<true, false>), grid, block, 0, st, a);
    } else {
        if (a.lookups) hipLaunchKernelGGL((k_occupancy_fuse<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_occupancy_fuse<false, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace sv
