// A world-fixed voxel map flattened into an occupancy map: include/stereo_vision_hip.h (V), restated in stereo_vision/sv.py
// (voxel_map_flatten).  The voxel map's buffer is voxel_map_kernels.h's and is only read; its filters, centre, height and head are
// voxel_map_table.h's, the flat map's geometry and cell rule are occupancy_map_cells.h's.  Four or five kernels in stream order;
// workgroups exchange data across the launch boundaries only:
//
//   clear    a lane per flat cell: last_seen, which holds `seen` until the last kernel, to -1; the three counts to 0; floor and top to
//            what the mode makes of them (below); the first lanes clear the stats (drawn = -1 for an overflowed map).
//   walk A   a strided walk of the table, a lane per slot and trip: the key, then n, m and last_seq for the filters - a word only where
//            the ones before it passed -, then the offset sums; the centre on axes 0 and 1, the flat cell, zq.  An atomic maximum of
//            last_seq on `seen`, and in mode 1 the cell's `low`: with radius 0 an atomic minimum of zq on floor, which is the base then;
//            with radius > 0 an atomic maximum of -2 - zq on top.  `drawn` and `outside` go by ballots, one add per workgroup.
//   floor    mode 1 with radius > 0 only: a workgroup per tile of 16 x 64 flat cells, the tile of top with a halo of `radius` cells in
//            LDS, a maximum along the rows, then along the columns: base = -2 - that, or -1 where the window holds no voxel, into floor.
//            No atomic.  It reads top and writes floor, so that no workgroup reads what another one writes.
//   walk B   the same walk and arithmetic; base = floor of the voxel's cell, the class of h = zq - base, an atomic add on one of the
//            cell's three counts and, for ground and obstacle, an atomic maximum of zq on top: zq >= 0 is above every word walk A left
//            there, which are all <= -2.  The four counts per class go by ballots, one add per workgroup.
//   resolve  a lane per flat cell: L and last_seen from the counts and `seen`; a floor still at its cleared word and a top still
//            negative become -1.  occupied_cells and free_cells go by ballots, summed per workgroup in LDS.
// Atomics are integer minima, maxima and adds only, none with a returned value, so the result is the same bits whatever the schedule.
//
// Bounds: a slot index is < slots (the walk); a flat cell comes from map_cell, which admits (r, c) inside rows x cols only, and its
// index r * cols + c is < rows * cols <= 8 000 000; the floor kernel reads top inside the map only - a halo cell outside it is the word of
// a cell without a voxel - and stores inside it only; the lanes of clear and resolve beyond rows * cols load and store nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_flatten_kernels.h"
#include "voxel_map_table.h"

namespace sv {

namespace {

constexpr int32_t VFLATTEN_NO_LOW = 0x7FFFFFFF;        // floor as `low`, radius 0: the minimum over no voxel
constexpr int32_t VFLATTEN_NO_LOW_TOP = -0x7FFFFFFF - 1;  // top as -2 - `low`, radius > 0: the maximum over no voxel
enum { VFLATTEN_DRAWN = 0, VFLATTEN_OUTSIDE = 1, VFLATTEN_BELOW = 2, VFLATTEN_OCCUPIED = 6, VFLATTEN_FREE = 7 };

__device__ __forceinline__ bool vflatten_windowed(const VoxelFlattenArgs &a) { return a.mode == 1 && a.radius > 0; }

__global__ __launch_bounds__(VFLATTEN_THREADS) void k_vflatten_clear(VoxelFlattenArgs a) {
    const int n_cells = a.m.rows * a.m.cols;
    const int i = (int)(blockIdx.x * VFLATTEN_THREADS + threadIdx.x);  // < 2^23 + 256
    if (i < VFLATTEN_STATS) a.stats[i] = i == VFLATTEN_DRAWN && vmap_overflowed_before(a.map) ? -1ll : 0ll;  // the grid has a workgroup at least
    if (i >= n_cells) return;
    a.last_seen[i] = -1;
    a.floor[i] = a.mode == 0 ? a.z_ref_q : VFLATTEN_NO_LOW;
    a.top[i] = vflatten_windowed(a) ? VFLATTEN_NO_LOW_TOP : -1;
#pragma unroll
    for (int k = 0; k < 3; k++) a.cells[3 * (size_t)i + k] = 0;
}

// PASS 0: walk A; PASS 1: walk B.
template <int PASS>
__global__ __launch_bounds__(VFLATTEN_THREADS) void k_vflatten_walk(VoxelFlattenArgs a) {
    __shared__ uint32_t s_count[VFLATTEN_THREADS / 64][4];
    if (vmap_overflowed_before(a.map)) return;  // the whole grid
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long *table = vmap_table(a.map);
    const size_t slots = (size_t)1 << a.log2_slots;  // a multiple of VFLATTEN_THREADS
    const bool windowed = vflatten_windowed(a);
    uint32_t count[4] = {0, 0, 0, 0};  // of this wavefront, over its trips - A: drawn, outside; B: below, ground, obstacle, overhead -: at most slots <= 2^27 each
    for (size_t slot = (size_t)blockIdx.x * VFLATTEN_THREADS + threadIdx.x; slot < slots; slot += (size_t)gridDim.x * VFLATTEN_THREADS) {  // the same trips for a workgroup
        const unsigned long long *e = table + slot * VMAP_ENTRY_WORDS;
        const unsigned long long key = e[VMAP_KEY];
        const bool live = key != VMAP_EMPTY && vmap_passes(a, e);
        if (!__ballot(live)) continue;  // the whole wavefront: no voxel on this trip
        bool inside = false;
        int cell = 0, zq = 0;
        if (live) {
            const unsigned long long n = e[VMAP_N];  // >= min_n >= 1
            const double X = vmap_centre(a.lo[0], a.size, key, 0, e[VMAP_S], n), Y = vmap_centre(a.lo[1], a.size, key, 1, e[VMAP_S + 1], n);
            int r, c;
            inside = map_cell(a.m, map_grid(a.m, X), map_grid(a.m, Y), r, c);
            if (inside) {
                cell = r * a.m.cols + c;  // < rows * cols
                zq = vmap_zq(key, 2, e[VMAP_S + 2], n);
            }
        }
        if (PASS == 0) {
            count[0] += (uint32_t)__popcll(__ballot(inside));  // every lane of the wavefront gets here
            count[1] += (uint32_t)__popcll(__ballot(live && !inside));
            if (inside) {
                atomicMax(a.last_seen + cell, (int32_t)vmap_last_seq(e[VMAP_SEQ]));
                if (windowed) atomicMax(a.top + cell, -2 - zq);
                else if (a.mode == 1) atomicMin(a.floor + cell, zq);
            }
        } else {
            int kind = -1;  // 0 below, 1 ground, 2 obstacle, 3 overhead
            if (inside) {
                const int h = zq - a.floor[cell];  // the cell holds a voxel: it has a base; |h| < 2^31
                kind = h < -a.step_q ? 0 : h < a.step_q ? 1 : h < a.height_q ? 2 : 3;
                if (kind > 0) atomicAdd(a.cells + 3 * (size_t)cell + (kind - 1), 1);
                if (kind == 1 || kind == 2) atomicMax(a.top + cell, zq);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) count[k] += (uint32_t)__popcll(__ballot(kind == k));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) s_count[wave][k] = count[k];
    }
    __syncthreads();  // every thread of the workgroup gets here
    const int k = (int)threadIdx.x;
    if (k >= (PASS == 0 ? 2 : 4)) return;
    uint32_t total = 0;
    for (int w = 0; w < VFLATTEN_THREADS / 64; w++) total += s_count[w][k];
    if (total) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + (PASS == 0 ? VFLATTEN_DRAWN : VFLATTEN_BELOW) + k, (unsigned long long)total);
}

// Mode 1, radius > 0.  grid (ceil(cols / 64), ceil(rows / 16)).
__global__ __launch_bounds__(VFLATTEN_THREADS) void k_vflatten_floor(VoxelFlattenArgs a) {
    constexpr int HR = VFLATTEN_TILE_ROWS + 2 * VFLATTEN_RADIUS_MAX, HC = VFLATTEN_TILE_COLS + 2 * VFLATTEN_RADIUS_MAX;
    __shared__ int32_t s_in[HR][HC];                  // the tile and its halo
    __shared__ int32_t s_row[HR][VFLATTEN_TILE_COLS];  // the maxima along the rows, for the tile's columns
    const int R = a.radius, rows = a.m.rows, cols = a.m.cols;
    const int r0 = (int)blockIdx.y * VFLATTEN_TILE_ROWS, c0 = (int)blockIdx.x * VFLATTEN_TILE_COLS;  // of the tile: inside the map
    const int hr = VFLATTEN_TILE_ROWS + 2 * R, hc = VFLATTEN_TILE_COLS + 2 * R;                      // <= HR, HC
    for (int i = (int)threadIdx.x; i < hr * hc; i += VFLATTEN_THREADS) {
        const int y = i / hc, x = i - y * hc;
        const int r = r0 - R + y, c = c0 - R + x;
        s_in[y][x] = (unsigned)r < (unsigned)rows && (unsigned)c < (unsigned)cols ? a.top[(size_t)r * cols + c] : VFLATTEN_NO_LOW_TOP;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < hr * VFLATTEN_TILE_COLS; i += VFLATTEN_THREADS) {
        const int y = i / VFLATTEN_TILE_COLS, x = i % VFLATTEN_TILE_COLS;
        int32_t best = VFLATTEN_NO_LOW_TOP;
        for (int d = 0; d <= 2 * R; d++) best = max(best, s_in[y][x + d]);  // x + d <= 63 + 2 R < hc
        s_row[y][x] = best;
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < VFLATTEN_TILE_ROWS * VFLATTEN_TILE_COLS; i += VFLATTEN_THREADS) {
        const int y = i / VFLATTEN_TILE_COLS, x = i % VFLATTEN_TILE_COLS;
        const int r = r0 + y, c = c0 + x;
        if (r >= rows || c >= cols) continue;
        int32_t best = VFLATTEN_NO_LOW_TOP;
        for (int d = 0; d <= 2 * R; d++) best = max(best, s_row[y + d][x]);  // y + d <= 15 + 2 R < hr
        a.floor[(size_t)r * cols + c] = best == VFLATTEN_NO_LOW_TOP ? -1 : -2 - best;
    }
}

__global__ __launch_bounds__(VFLATTEN_THREADS) void k_vflatten_resolve(VoxelFlattenArgs a) {
    __shared__ uint32_t s_count[VFLATTEN_THREADS / 64][2];  // occupied, free
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n_cells = a.m.rows * a.m.cols;
    const int i = (int)(blockIdx.x * VFLATTEN_THREADS + threadIdx.x);
    int state = 0;  // 1 free, 2 occupied
    if (i < n_cells) {
        const int ground = a.cells[3 * (size_t)i], obstacle = a.cells[3 * (size_t)i + 1];
        long long L = 0;
        if (obstacle >= a.min_obstacle) {
            L = (long long)obstacle * a.l_occ;
            L = L < a.l_max ? L : a.l_max;
            state = 2;
        } else if (ground >= a.min_ground) {
            L = -((long long)ground * a.l_free);
            L = L > a.l_min ? L : a.l_min;
            state = 1;
        }
        a.logodds[i] = (int16_t)L;  // l_min .. l_max
        if (!state) a.last_seen[i] = -1;
        if (a.floor[i] == VFLATTEN_NO_LOW) a.floor[i] = -1;  // |z_ref_q| < 2^30 is never this word
        if (a.top[i] < 0) a.top[i] = -1;
    }
    // every lane of the workgroup gets here
    const uint32_t n_occupied = (uint32_t)__popcll(__ballot(state == 2)), n_free = (uint32_t)__popcll(__ballot(state == 1));
    if (lane == 0) s_count[wave][0] = n_occupied, s_count[wave][1] = n_free;
    __syncthreads();
    const int k = (int)threadIdx.x;
    if (k >= 2) return;
    uint32_t total = 0;
    for (int w = 0; w < VFLATTEN_THREADS / 64; w++) total += s_count[w][k];
    if (total) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + VFLATTEN_OCCUPIED + k, (unsigned long long)total);
}

}  // namespace

hipError_t launch_voxel_flatten(const VoxelFlattenArgs &a, int max_groups, int stages, hipStream_t st) {
    if (max_groups < 1 || max_groups > VFLATTEN_MAX_GROUPS || stages < 0 || stages >= VFLATTEN_STAGES) return hipErrorInvalidValue;
    const unsigned per_cell = (unsigned)(((size_t)a.m.rows * a.m.cols + VFLATTEN_THREADS - 1) / VFLATTEN_THREADS);  // >= 1
    hipLaunchKernelGGL(k_vflatten_clear, dim3(per_cell), dim3(VFLATTEN_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (stages == 1) return hipSuccess;
    const size_t tiles = ((size_t)1 << a.log2_slots) / VFLATTEN_THREADS;  // slots is a multiple of 1024
    const dim3 walk((unsigned)(tiles < (size_t)max_groups ? tiles : (size_t)max_groups));
    hipLaunchKernelGGL(k_vflatten_walk<0>, walk, dim3(VFLATTEN_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (stages == 2) return hipSuccess;
    if (a.mode == 1 && a.radius > 0) {
        const dim3 grid((unsigned)((a.m.cols + VFLATTEN_TILE_COLS - 1) / VFLATTEN_TILE_COLS), (unsigned)((a.m.rows + VFLATTEN_TILE_ROWS - 1) / VFLATTEN_TILE_ROWS));
        hipLaunchKernelGGL(k_vflatten_floor, grid, dim3(VFLATTEN_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    if (stages == 3) return hipSuccess;
    hipLaunchKernelGGL(k_vflatten_walk<1>, walk, dim3(VFLATTEN_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (stages == 4) return hipSuccess;
    hipLaunchKernelGGL(k_vflatten_resolve, dim3(per_cell), dim3(VFLATTEN_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
