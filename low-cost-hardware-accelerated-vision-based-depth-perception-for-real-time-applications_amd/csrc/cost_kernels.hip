// The penalties, the cost-to-goal field and the routes of the world map: include/stereo_vision_hip.h (N), restated in stereo_vision/sv.py
// (cost_cells, cost_to_goal, cost_routes).  Integers throughout: minima of sums, which do not depend on any order.  No atomics on the
// results, no exchange between workgroups inside a launch, and no loop without a bound fixed at launch.
//
//   cells   element-wise, 16 cells a thread: two 16-byte loads of d2 and one 16-byte store of pen where both arrays are 16-byte aligned,
//           cell by cell elsewhere and in the last chunk.  The root is a compare ladder of eight steps: no floating point.
//
//   fill, seed   the start of a field: COST_INF in both cost buffers and 0 in both sets of dirty bytes; then - a launch later - 0 in
//           both buffers on every goal that is inside the map and free, and 1 in the dirty byte of its tile.  Several goals may store
//           into one word: all of them store the same value.
//
//   sweep   a workgroup per tile of 64 x 64 cells.  It asks the dirty bytes of the sweep before whether it or one of its 8 neighbour
//           tiles changed then; if none did it stores its own 0 byte and is done - the field needs no store, see k_cost_sweep.  Else it
//           stages cost and pen of 66 x 66 cells (COST_INF and blocked outside the map), makes per cell the 8 bits of its admissible moves
//           once, and relaxes Jacobi-wise between two LDS copies - a thread owns 16 consecutive rows of one column and slides a 3 x 3
//           window of registers down them - until an iteration changes nothing in the tile (__syncthreads_or) or COST_INNER_MAX is
//           reached.  It writes the tile to the OTHER global buffer, 1 or 0 to its byte of the next sweep's dirty bytes and, where it
//           changed, 1 to the sweep's word: a plain store, every writer the same value.
//
//   info    one wavefront counts the sweeps' words of the call.
//
//   routes  8 lanes per route, one neighbour each, 8 routes per wavefront; the least cost[b] + step of the group and the lowest lane that
//           has it by three xor shuffles of (value << 3 | lane).  Every lane stays in the loop until all routes of its wavefront have
//           stopped, so no shuffle is made under divergence; the loop's bound is capacity.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cost_kernels.h"
#include "wave_ops.h"

namespace sv {

// The move a route's lane j or a mask's bit j stands for, in the order the tie rule names: four axial moves, then four diagonal ones.
__device__ __forceinline__ int cost_move_dr(int j) { return j < 4 ? (j == 0 ? -1 : j == 3 ? 1 : 0) : (j < 6 ? -1 : 1); }
__device__ __forceinline__ int cost_move_dc(int j) { return j < 4 ? (j == 1 ? -1 : j == 2 ? 1 : 0) : ((j & 1) ? 1 : -1); }
__device__ __forceinline__ int cost_move_step(int j) { return j < 4 ? (int)COST_STEP_AXIAL : (int)COST_STEP_DIAGONAL; }

__device__ __forceinline__ uint32_t cost_pen_of(uint32_t v, const CostCellsArgs &a) {
    if ((int)v <= a.r2_block) return COST_BLOCKED;
    uint32_t root = 0;  // floor(sqrt(v)), v < 2^16: a bit stays where the square does not exceed v
#pragma unroll
    for (uint32_t b = 128; b >= 1; b >>= 1) {
        const uint32_t t = root | b;
        root = t * t <= v ? t : root;
    }
    // v = 65535 has root 255 > soft: 0 without a branch
    return min((uint32_t)COST_PEN_MAX, (uint32_t)a.weight * (uint32_t)max(0, a.soft - (int)root));
}

__global__ __launch_bounds__(COST_THREADS) void k_cost_cells(CostCellsArgs a) {
    const bool wide = ((reinterpret_cast<uintptr_t>(a.d2) | reinterpret_cast<uintptr_t>(a.pen)) & 15) == 0;  // uniform
    const int64_t stride = (int64_t)gridDim.x * COST_THREADS * 16;
    for (int64_t base = ((int64_t)blockIdx.x * COST_THREADS + threadIdx.x) * 16; base < a.cells; base += stride) {
        if (wide && base + 16 <= a.cells) {
            const uint4 lo = *reinterpret_cast<const uint4 *>(a.d2 + base), hi = *reinterpret_cast<const uint4 *>(a.d2 + base + 8);
            const uint32_t in[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            uint32_t out[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                out[k] = cost_pen_of(in[2 * k] & 0xFFFFu, a) | cost_pen_of(in[2 * k] >> 16, a) << 8 | cost_pen_of(in[2 * k + 1] & 0xFFFFu, a) << 16 |
                         cost_pen_of(in[2 * k + 1] >> 16, a) << 24;
            *reinterpret_cast<uint4 *>(a.pen + base) = make_uint4(out[0], out[1], out[2], out[3]);
        } else {
            const int n = (int)min((int64_t)16, a.cells - base);
            for (int k = 0; k < n; k++) a.pen[base + k] = (uint8_t)cost_pen_of(a.d2[base + k], a);
        }
    }
}

__global__ __launch_bounds__(COST_THREADS) void k_cost_fill(CostFieldArgs a) {
    const int64_t cells = (int64_t)a.rows * a.cols, tiles = (int64_t)a.tiles_x * a.tiles_y, stride = (int64_t)gridDim.x * COST_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * COST_THREADS + threadIdx.x; i < cells; i += stride) a.cost[i] = COST_INF, a.twin[i] = COST_INF;
    for (int64_t i = (int64_t)blockIdx.x * COST_THREADS + threadIdx.x; i < tiles; i += stride) a.dirty[0][i] = 0, a.dirty[1][i] = 0;
}

__global__ __launch_bounds__(COST_THREADS) void k_cost_seed(CostFieldArgs a) {
    const int k = (int)blockIdx.x * COST_THREADS + (int)threadIdx.x;
    if (k >= a.n_goals) return;  // no barrier in this kernel
    const int r = a.goals[2 * k], c = a.goals[2 * k + 1];
    if ((unsigned)r >= (unsigned)a.rows || (unsigned)c >= (unsigned)a.cols) return;
    const size_t g = (size_t)r * a.cols + c;
    if (a.pen[g] == COST_BLOCKED) return;
    a.cost[g] = 0, a.twin[g] = 0;
    a.dirty[0][(r / COST_TILE) * a.tiles_x + c / COST_TILE] = 1;  // the first sweep reads dirty[0]
}

// The 8 bits of the admissible moves of the staged cell at s_pen[at]; 0 for a blocked one.
__device__ __forceinline__ uint32_t cost_moves_of(const uint8_t *s_pen, int at) {
    if (s_pen[at] == COST_BLOCKED) return 0;
    uint32_t free9 = 0;  // bit (dr + 1) * 3 + dc + 1
#pragma unroll
    for (int dr = -1; dr <= 1; dr++)
#pragma unroll
        for (int dc = -1; dc <= 1; dc++) free9 |= (uint32_t)(s_pen[at + dr * COST_SIDE + dc] != COST_BLOCKED) << ((dr + 1) * 3 + dc + 1);
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int dr = cost_move_dr(j), dc = cost_move_dc(j);
        const uint32_t need = 1u << ((dr + 1) * 3 + dc + 1) | 1u << ((dr + 1) * 3 + 1) | 1u << (3 + dc + 1);  // b and, diagonally, the corner's two
        m |= (uint32_t)((free9 & need) == need) << j;
    }
    return m;
}

template <bool COUNT>
__global__ __launch_bounds__(COST_THREADS) void k_cost_sweep(CostFieldArgs a, int sweep) {
    enum { ROWS_PER_THREAD = COST_TILE * COST_TILE / COST_THREADS };  // 16: a thread owns rows wave * 16 .. + 15 of column lane
    __shared__ int32_t s_cost[2][COST_SIDE * COST_SIDE];
    __shared__ uint8_t s_pen[COST_SIDE * COST_SIDE];
    const int tid = (int)threadIdx.x, tx = (int)blockIdx.x, ty = (int)blockIdx.y, tile = ty * a.tiles_x + tx;
    const uint8_t *dirty_in = a.dirty[sweep & 1];
    uint8_t *dirty_out = a.dirty[(sweep + 1) & 1];
    const int32_t *in = (sweep & 1) ? a.twin : a.cost;
    int32_t *out = (sweep & 1) ? a.cost : a.twin;

    // Did this tile or one of its 8 neighbours change in the sweep before?  dirty_in was written by the launch before this one.
    int near = 0;
    if (tid < 9) {
        const int nx = tx + tid % 3 - 1, ny = ty + tid / 3 - 1;
        if (nx >= 0 && nx < a.tiles_x && ny >= 0 && ny < a.tiles_y) near = dirty_in[ny * a.tiles_x + nx];
    }
    if (!(__syncthreads_or(near) | a.all_tiles)) {  // the same for every thread: all of them leave here, or none
        // Nothing is written to `out`: this tile did not change in the sweep before, so what that sweep left of it in `in` equals what
        // `out` already holds - either it ran then and wrote `in` = its input, or it did not run and the two were equal before (by
        // induction from k_cost_fill, which makes them equal).  Only its byte of the next sweep's dirty set is cleared.
        if (tid == 0) dirty_out[tile] = 0;
        return;
    }

    const int r0 = ty * COST_TILE, c0 = tx * COST_TILE;
    for (int i = tid; i < COST_SIDE * COST_SIDE; i += COST_THREADS) {
        const int r = r0 - 1 + i / COST_SIDE, c = c0 - 1 + i % COST_SIDE;
        const bool inside = r >= 0 && r < a.rows && c >= 0 && c < a.cols;  // outside the map: blocked, the edge is a wall
        const size_t g = (size_t)(inside ? r : 0) * a.cols + (inside ? c : 0);
        const int32_t v = inside ? in[g] : COST_INF;
        s_pen[i] = inside ? a.pen[g] : (uint8_t)COST_BLOCKED;
        s_cost[0][i] = v, s_cost[1][i] = v;  // the halo is the same in both copies and is never written again
    }
    __syncthreads();

    const int lane = tid & 63, y0 = (tid >> 6) * ROWS_PER_THREAD;
    const int top = (y0 + 1) * COST_SIDE + lane + 1;  // the thread's first cell among the staged ones
    uint32_t moves[ROWS_PER_THREAD / 4], pens[ROWS_PER_THREAD / 4];  // a byte per cell; every index below is a constant after unrolling
#pragma unroll
    for (int k = 0; k < ROWS_PER_THREAD / 4; k++) moves[k] = 0, pens[k] = 0;
#pragma unroll
    for (int k = 0; k < ROWS_PER_THREAD; k++) {
        moves[k >> 2] |= cost_moves_of(s_pen, top + k * COST_SIDE) << (8 * (k & 3));
        pens[k >> 2] |= (uint32_t)s_pen[top + k * COST_SIDE] << (8 * (k & 3));
    }

    // Jacobi between the two copies: an iteration reads s_cost[cur] only and writes the cells of s_cost[cur ^ 1] only, each by its owner;
    // the barrier of __syncthreads_or ends it, and its verdict is the same in every thread.
    int cur = 0, changed = 0, iterations = 0;
    for (int it = 0; it < COST_INNER_MAX; it++) {
        const int32_t *src = s_cost[cur];
        int32_t *dst = s_cost[cur ^ 1];
        uint32_t w[3][3];  // the rows above, of and below the cell, columns lane - 1 .. lane + 1
#pragma unroll
        for (int x = 0; x < 3; x++) w[0][x] = (uint32_t)src[top - COST_SIDE - 1 + x], w[1][x] = (uint32_t)src[top - 1 + x];
        int mine = 0;
#pragma unroll
        for (int k = 0; k < ROWS_PER_THREAD; k++) {
            const int at = top + k * COST_SIDE;
#pragma unroll
            for (int x = 0; x < 3; x++) w[2][x] = (uint32_t)src[at + COST_SIDE - 1 + x];
            const uint32_t m = moves[k >> 2] >> (8 * (k & 3)) & 255u, pen = pens[k >> 2] >> (8 * (k & 3)) & 255u, old = w[1][1];
            uint32_t best = ~0u;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                // COST_INF + step is above COST_INF as an unsigned word, a finite cost + step + pen stays below it (COST_CELLS_MAX)
                const uint32_t v = w[1 + cost_move_dr(j)][1 + cost_move_dc(j)] + (uint32_t)cost_move_step(j);
                best = min(best, (m >> j & 1u) ? v : ~0u);
            }
            const uint32_t now = best < (uint32_t)COST_INF ? min(old, best + pen) : old;
            dst[at] = (int32_t)now;
            mine |= now != old;
#pragma unroll
            for (int x = 0; x < 3; x++) w[0][x] = w[1][x], w[1][x] = w[2][x];
        }
        cur ^= 1;
        iterations++;
        const int go = __syncthreads_or(mine);
        changed |= go;
        if (!go) break;
    }

    const int c = c0 + lane;
    if (c < a.cols)
#pragma unroll
        for (int k = 0; k < ROWS_PER_THREAD; k++) {
            const int r = r0 + y0 + k;
            if (r < a.rows) out[(size_t)r * a.cols + c] = s_cost[cur][top + k * COST_SIDE];  // the thread's own cells: no barrier needed
        }
    if (tid == 0) {
        dirty_out[tile] = changed ? 1 : 0;
        if (changed) a.changed[sweep] = 1;
        if (COUNT) atomicAdd(a.counters, 1ull), atomicAdd(a.counters + 1, (unsigned long long)iterations);
    }
}

__global__ __launch_bounds__(64) void k_cost_info(CostFieldArgs a, int sweeps) {
    const int lane = (int)threadIdx.x;
    int n = 0;
    for (int s = lane; s < sweeps; s += 64) n += a.changed[s] != 0;
    n = wave_sum(n);
    if (lane == 0) a.info[0] = a.changed[sweeps - 1] != 0, a.info[1] = n, a.info[2] = 0, a.info[3] = 0;
}

__global__ __launch_bounds__(COST_THREADS) void k_cost_routes(CostRoutesArgs a) {
    const int tid = (int)threadIdx.x, j = tid & (COST_ROUTE_LANES - 1);
    const int route = ((int)blockIdx.x * COST_THREADS + tid) / COST_ROUTE_LANES;
    const int dr = cost_move_dr(j), dc = cost_move_dc(j), step = cost_move_step(j);
    const bool have = route < a.n_routes;
    int r = 0, c = 0, n = 0, status = 0;
    bool active = false;
    if (have) {
        r = a.starts[2 * route], c = a.starts[2 * route + 1];
        if ((unsigned)r >= (unsigned)a.rows || (unsigned)c >= (unsigned)a.cols) status = 1;
        else if (a.pen[(size_t)r * a.cols + c] == COST_BLOCKED || a.cost[(size_t)r * a.cols + c] == COST_INF) status = 2;
        else active = true;
    }
    int16_t *cells = a.cells + (size_t)(have ? route : 0) * a.capacity * 2;
    for (int it = 0; it < a.capacity; it++) {
        if (!__any(active)) break;  // the same in every lane of the wavefront: the shuffles below are reached by all of them or by none
        int here = 0;
        unsigned long long key = ~0ull;  // (cost[b] + step) << 3 | lane of the group; ~0 for no admissible neighbour with a finite cost
        if (active) {
            here = a.cost[(size_t)r * a.cols + c];
            if (j == 0) *reinterpret_cast<short2 *>(cells + 2 * (size_t)n) = make_short2((short)r, (short)c);
            const int nr = r + dr, nc = c + dc;
            if (here != 0 && (unsigned)nr < (unsigned)a.rows && (unsigned)nc < (unsigned)a.cols && a.pen[(size_t)nr * a.cols + nc] != COST_BLOCKED &&
                (j < 4 || (a.pen[(size_t)r * a.cols + nc] != COST_BLOCKED && a.pen[(size_t)nr * a.cols + c] != COST_BLOCKED))) {
                const int32_t v = a.cost[(size_t)nr * a.cols + nc];
                if (v != COST_INF) key = (unsigned long long)((uint32_t)v + (uint32_t)step) << 3 | (unsigned)j;
            }
        }
        // the minimum over the 8 lanes of a group - wave_ops.h's butterfly cut off at the group's width, so written out here; ties go
        // to the lowest lane, the first move of the order
#pragma unroll
        for (int off = COST_ROUTE_LANES / 2; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(key, off, 64);
            key = o < key ? o : key;
        }
        if (active) {
            n++;
            const int jb = (int)(key & 7ull);
            if (here == 0) {
                active = false;  // status 0: a goal
            } else if (key == ~0ull || (long long)(key >> 3) - cost_move_step(jb) >= (long long)here) {
                status = 4, active = false;  // not downhill: the field is no fixed point here
            } else if (n == a.capacity) {
                status = 3, active = false;
            } else {
                r += cost_move_dr(jb), c += cost_move_dc(jb);
            }
        }
    }
    if (have && j == 0) a.length[route] = n, a.status[route] = status;
}

hipError_t launch_cost_cells(const CostCellsArgs &a, hipStream_t st) {
    const int64_t chunks = (a.cells + 15) / 16;
    const unsigned blocks = (unsigned)min((int64_t)2048, (chunks + COST_THREADS - 1) / COST_THREADS);
    hipLaunchKernelGGL(k_cost_cells, dim3(blocks), dim3(COST_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_cost_to_goal(const CostFieldArgs &a, int init, int sweeps, hipStream_t st) {
    // the sweeps' words: a block of their own at the workspace's start, 16-byte aligned and a multiple of 16 bytes
    hipError_t e = hipMemsetAsync(a.changed, 0, COST_SWEEPS_MAX * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    if (init) {
        const int64_t cells = (int64_t)a.rows * a.cols;
        hipLaunchKernelGGL(k_cost_fill, dim3((unsigned)min((int64_t)2048, (cells + COST_THREADS - 1) / COST_THREADS)), dim3(COST_THREADS), 0, st, a);
        hipLaunchKernelGGL(k_cost_seed, dim3((a.n_goals + COST_THREADS - 1) / COST_THREADS), dim3(COST_THREADS), 0, st, a);
    }
    const dim3 grid(a.tiles_x, a.tiles_y);
    for (int s = 0; s < sweeps; s++) {
        if (a.counters) hipLaunchKernelGGL(k_cost_sweep<true>, grid, dim3(COST_THREADS), 0, st, a, s);
        else hipLaunchKernelGGL(k_cost_sweep<false>, grid, dim3(COST_THREADS), 0, st, a, s);
    }
    hipLaunchKernelGGL(k_cost_info, dim3(1), dim3(64), 0, st, a, sweeps);
    return hipGetLastError();
}

hipError_t launch_cost_routes(const CostRoutesArgs &a, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.cells, 0xFF, (size_t)a.n_routes * a.capacity * 2 * sizeof(int16_t), st);  // -1 in every cell
    if (e != hipSuccess) return e;
    const int per_block = COST_THREADS / COST_ROUTE_LANES;
    hipLaunchKernelGGL(k_cost_routes, dim3((a.n_routes + per_block - 1) / per_block), dim3(COST_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
