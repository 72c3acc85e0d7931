// The frontier cells and the frontier clusters of the world map: include/stereo_vision_hip.h (O), restated in stereo_vision/sv.py
// (frontier_cells, frontier_clusters).  Integers throughout.  A label is the least linear index of its 8-connected component - a function
// of the partition alone - and every statistic is a sum, a minimum or a maximum of integers: the same bits whatever order the unions and
// the atomics take.
//
//   cells    a workgroup owns FRONTIER_SPAN consecutive cells of the map taken as one line.  It decides the state of every cell it needs
//            once and stages it as a byte in LDS: its own cells with one cell before and behind them and - where a row has at most
//            FRONTIER_HALO_COLS cells - the row above and the row below, which lie `cols` cells before and behind in the same line.  With
//            longer rows the states above and below are decided from global memory where a free cell asks for them.  The state is
//            occupancy_map_cells.h's, as the view decides it.  Chunks of 16 cells: that header's wide loader where logodds and last_seen
//            are 16-byte aligned, one 16-byte load of pen and one 16-byte store of the mask where those are; cell by cell elsewhere, in
//            a cut chunk and outside the map.
//
//   tiles    a workgroup of 256 threads per tile of 64 x 64 cells: a union-find over the tile in LDS.  Every member starts as its own
//            parent and unites with its W, NW, N and NE neighbours inside the tile; after a barrier each member looks its root up and
//            writes the root's GLOBAL index to parent[] (-1 on non-members).  Row-major order inside a tile agrees with the global
//            linear order, so a tile-local root is the least global index of its piece.  A tile without a member writes its -1s and
//            leaves - all of its threads, after the same barrier.
//
//   seams    a thread per cell of the first row and the first column of every tile.  A member there unites with its neighbours over the
//            seam: N, NW and NE for the first row (the NW and NE of the row's ends lie in the diagonal tiles: the four corner diagonals),
//            W, NW and SW for the first column, where the corner's NW belongs to the row's rule and the last cell's SW is the NE of a
//            first-row cell of the tile below.  Every adjacency between two tiles is covered exactly once.
//
//            THIS IS THE ONLY LAUNCH IN WHICH A WORKGROUP READS A WORD THAT ANOTHER WORKGROUP MAY WRITE IN THE SAME LAUNCH.  In it every
//            access to parent[] is a relaxed agent-scope atomic (__hip_atomic_load / __hip_atomic_fetch_min with
//            __HIP_MEMORY_SCOPE_AGENT): a plain load could be served by the CU's L1 or the XCD's L2, which are not coherent for it.
//            There is no cooperative launch, no grid barrier, no flag, and no loop that waits for a value another thread has yet to
//            write: a thread only ever reacts to what it has read, and whatever it reads lets it go on.
//
//   flatten  label[i] = find(i), read from parent[] (written by the launches before) and written to label[]: nothing read here is
//            written in this launch.  The member count of a component is added at its root's word of size[]; runs of equal labels in
//            consecutive lanes are combined (wave_run), so one lane issues a run's atomic.
//
//   count, scan, rank   the ordered compaction of the kept roots (label == own index, size >= min_cells), as the compact clouds do it: a
//            wavefront owns 1024 consecutive cells in both big kernels, counts by ballots, one workgroup scans the counts and writes
//            info, and the rank kernel gives a kept root the row of its rank - initialised if the rank is below capacity - and leaves
//            the rank, or -1, where the root's count was.
//
//   stats, keys, reps   every member whose root has a rank adds its row and column into sums (64-bit atomicAdd) and takes part in the
//            box's atomicMin / atomicMax; a launch later it atomicMins the key d2 << 23 | index of the representative; a last small
//            kernel decodes the key.  Both combine the runs of equal ranks in consecutive lanes first.
//
// Every other exchange between workgroups happens across a launch boundary.  No shuffle runs under divergence - the lanes without data
// pass a neutral value to the same call - and no barrier sits in a branch that some thread of the workgroup skips.  A tile, a seam cell
// or a thread past the map's edge takes the neutral path to the same barriers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frontier_kernels.h"
#include "occupancy_map_cells.h"
#include "wave_ops.h"

namespace sv {

namespace {

enum { FRONTIER_WAVE_CELLS = 1024 };  // the cells one wavefront counts and ranks: 16 sweeps of 64

// ---- the union-find in LDS (tiles) -----------------------------------------------------------------------------------------------

__device__ __forceinline__ int lds_load(const int32_t *p, int x) { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Ends by the data alone: a parent is below its child, so the chain strictly descends and stops at a root.
__device__ __forceinline__ int lds_find(const int32_t *p, int x) {
    for (;;) {
        const int q = lds_load(p, x);
        if (q == x) return x;
        x = q;
    }
}

// Hooks the larger root under the smaller.  Ends by the data alone: the loop comes round again only when the word it aimed at had been
// lowered by another thread in the meantime (old != a), and the words of a tile can be lowered only finitely often.
__device__ __forceinline__ void lds_unite(int32_t *p, int a, int b) {
    for (;;) {
        a = lds_find(p, a), b = lds_find(p, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;  // a was still a root: hooked
        a = old;               // a had a parent already; min(old, b) is its parent now, and old and b are still to be united
    }
}

// ---- the union-find in global memory (seams): relaxed agent-scope atomics only ----------------------------------------------------

__device__ __forceinline__ int agent_load(const int32_t *p, int x) { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Ends by the data alone: parents strictly descend along a chain, whatever other threads lower meanwhile.
__device__ __forceinline__ int agent_find(const int32_t *p, int x) {
    for (;;) {
        const int q = agent_load(p, x);
        if (q == x) return x;
        x = q;
    }
}

// As lds_unite; returns the fetch_mins it issued.  Ends by the data alone: a retry follows only a fetch_min that found its word lowered
// by another thread, which can happen only finitely often - every lowering takes a word of parent[] strictly down, and none goes below 0.
__device__ __forceinline__ int agent_unite(int32_t *p, int a, int b) {
    int issued = 0;
    for (;;) {
        a = agent_find(p, a), b = agent_find(p, b);
        if (a == b) return issued;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        issued++;
        if (old == a) return issued;
        a = old;
    }
}

// Unites member i with cell j if that is a member; j is inside the map.  A non-member's word is -1 in every launch and never changes.
__device__ __forceinline__ int seam_link(int32_t *p, int i, int j) { return agent_load(p, j) >= 0 ? agent_unite(p, i, j) : 0; }

}  // namespace

__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_cells(FrontierCellsArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t s_state[FRONTIER_SPAN + 2 * FRONTIER_HALO_COLS];
    const int tid = (int)threadIdx.x;
    const int64_t cells = (int64_t)a.rows * a.cols, b0 = (int64_t)blockIdx.x * FRONTIER_SPAN;
    const bool rows_staged = a.cols <= FRONTIER_HALO_COLS;  // uniform
    const int halo = rows_staged ? (a.cols + FRONTIER_CHUNK - 1) / FRONTIER_CHUNK * FRONTIER_CHUNK : FRONTIER_CHUNK;  // whole chunks: <= FRONTIER_HALO_COLS
    const int64_t lo = b0 - halo;  // s_state[k] is the state of cell lo + k; b0 and halo are multiples of 16, so is lo
    const int n_chunks = (FRONTIER_SPAN + 2 * halo) / FRONTIER_CHUNK;
    const bool wide_in = ((reinterpret_cast<uintptr_t>(a.logodds) | reinterpret_cast<uintptr_t>(a.last_seen)) & 15) == 0;  // uniform

    // the state of every staged cell, decided once; a cell outside the map is not unknown (2: neither free nor unknown)
    for (int ch = tid; ch < n_chunks; ch += FRONTIER_THREADS) {
        const int64_t g = lo + (int64_t)ch * FRONTIER_CHUNK;
        uint32_t w[4] = {0, 0, 0, 0};
        if (wide_in && g >= 0 && g + FRONTIER_CHUNK <= cells) {
            map_state16(a.logodds + g, a.last_seen + g, a.occupied, a.free_, w);
        } else {
#pragma unroll
            for (int k = 0; k < FRONTIER_CHUNK; k++) {
                const int64_t i = g + k;
                uint32_t st = 2;
                if (i >= 0 && i < cells) st = map_state(a.logodds[i], a.last_seen[i], a.occupied, a.free_);
                w[k >> 2] |= st << (8 * (k & 3));
            }
        }
        *reinterpret_cast<uint4 *>(s_state + ch * FRONTIER_CHUNK) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();  // every thread: the loop above has no exit of its own

    const bool wide_out = ((reinterpret_cast<uintptr_t>(a.mask) | reinterpret_cast<uintptr_t>(a.pen)) & 15) == 0;  // uniform; a NULL pen is aligned
    for (int ch = tid; ch < FRONTIER_SPAN / FRONTIER_CHUNK; ch += FRONTIER_THREADS) {
        const int64_t g = b0 + (int64_t)ch * FRONTIER_CHUNK;
        if (g >= cells) break;  // no barrier below
        const bool whole = wide_out && g + FRONTIER_CHUNK <= cells;
        uint32_t pw[4] = {0, 0, 0, 0};  // pen of the chunk; 0 = free where there is no pen
        if (whole && a.pen) {
            const uint4 p = *reinterpret_cast<const uint4 *>(a.pen + g);
            pw[0] = p.x, pw[1] = p.y, pw[2] = p.z, pw[3] = p.w;
        }
        const int n = (int)min((int64_t)FRONTIER_CHUNK, cells - g);
        int c = (int)(g % a.cols);
        uint32_t out[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < FRONTIER_CHUNK; k++) {
            if (k < n) {
                const int64_t i = g + k;
                const int at = (int)(i - lo);
                uint32_t m = 0;
                if (s_state[at] == 1) {
                    bool unknown = (c > 0 && s_state[at - 1] == 0) || (c + 1 < a.cols && s_state[at + 1] == 0);
                    if (i >= a.cols) unknown |= (rows_staged ? (uint32_t)s_state[at - a.cols] : map_state(a.logodds[i - a.cols], a.last_seen[i - a.cols], a.occupied, a.free_)) == 0;
                    if (i + a.cols < cells) unknown |= (rows_staged ? (uint32_t)s_state[at + a.cols] : map_state(a.logodds[i + a.cols], a.last_seen[i + a.cols], a.occupied, a.free_)) == 0;
                    if (unknown) {
                        const uint32_t pen = !a.pen ? 0u : whole ? (pw[k >> 2] >> (8 * (k & 3)) & 255u) : (uint32_t)a.pen[i];
                        m = pen != FRONTIER_BLOCKED;
                    }
                }
                if (whole) out[k >> 2] |= m << (8 * (k & 3));
                else a.mask[i] = (uint8_t)m;
                c = c + 1 == a.cols ? 0 : c + 1;
            }
        }
        if (whole) *reinterpret_cast<uint4 *>(a.mask + g) = make_uint4(out[0], out[1], out[2], out[3]);
    }
}

template <bool COUNT>
__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_tiles(FrontierArgs a) {
    enum { PER_THREAD = FRONTIER_TILE * FRONTIER_TILE / FRONTIER_THREADS };  // 16: a thread owns the cells k * 256 + tid of the tile, row-major
    __shared__ int32_t s_parent[FRONTIER_TILE * FRONTIER_TILE];
    const int tid = (int)threadIdx.x, r0 = (int)blockIdx.y * FRONTIER_TILE, c0 = (int)blockIdx.x * FRONTIER_TILE;
    uint32_t mine = 0;  // bit k: the thread's k-th cell is a member
#pragma unroll
    for (int k = 0; k < PER_THREAD; k++) {
        const int li = k * FRONTIER_THREADS + tid, r = r0 + (li >> 6), c = c0 + (li & 63);
        const bool member = r < a.rows && c < a.cols && a.mask[(size_t)r * a.cols + c] != 0;  // past the map's edge: no member
        s_parent[li] = member ? li : -1;
        mine |= (uint32_t)member << k;
    }
    if (!__syncthreads_or((int)mine)) {  // the same for every thread: all of them leave here, or none
#pragma unroll
        for (int k = 0; k < PER_THREAD; k++) {
            const int li = k * FRONTIER_THREADS + tid, r = r0 + (li >> 6), c = c0 + (li & 63);
            if (r < a.rows && c < a.cols) a.parent[(size_t)r * a.cols + c] = -1;
        }
        return;
    }
    // The barrier above also published s_parent.  From here to the next barrier its words are read and lowered by LDS atomics only.
    for (int k = 0; k < PER_THREAD; k++) {
        if (!(mine >> k & 1u)) continue;
        const int li = k * FRONTIER_THREADS + tid, lr = li >> 6, lc = li & 63;
        if (lc > 0 && lds_load(s_parent, li - 1) >= 0) lds_unite(s_parent, li, li - 1);
        if (lr > 0) {
            if (lc > 0 && lds_load(s_parent, li - FRONTIER_TILE - 1) >= 0) lds_unite(s_parent, li, li - FRONTIER_TILE - 1);
            if (lds_load(s_parent, li - FRONTIER_TILE) >= 0) lds_unite(s_parent, li, li - FRONTIER_TILE);
            if (lc < FRONTIER_TILE - 1 && lds_load(s_parent, li - FRONTIER_TILE + 1) >= 0) lds_unite(s_parent, li, li - FRONTIER_TILE + 1);
        }
    }
    __syncthreads();  // every thread: the loop above only skips cells
#pragma unroll 4
    for (int k = 0; k < PER_THREAD; k++) {
        const int li = k * FRONTIER_THREADS + tid, r = r0 + (li >> 6), c = c0 + (li & 63);
        if (r < a.rows && c < a.cols) {
            int32_t v = -1;
            if (mine >> k & 1u) {
                const int root = lds_find(s_parent, li);  // nothing is written any more
                v = (r0 + (root >> 6)) * a.cols + c0 + (root & 63);
            }
            a.parent[(size_t)r * a.cols + c] = v;
        }
    }
    if (COUNT && tid == 0) atomicAdd(a.counters + 1, 1ull);
}

// Without the tile phase: every member its own parent.
__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_init(FrontierArgs a) {
    const int cells = a.rows * a.cols, i = (int)blockIdx.x * FRONTIER_THREADS + (int)threadIdx.x;
    if (i < cells) a.parent[i] = a.mask[i] != 0 ? i : -1;
}

// ALL = false: a thread per cell of the first row and the first column of a tile; ALL = true: a thread per cell of the map, with its four
// backward neighbours.  Every access to parent[] in this kernel is a relaxed agent-scope atomic - see the head of the file.  No barrier
// and no shuffle: a thread without work returns.
template <bool ALL, bool COUNT>
__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_seams(FrontierArgs a) {
    const int t = (int)blockIdx.x * FRONTIER_THREADS + (int)threadIdx.x;
    int r, c;
    bool over_row, over_col, corner = false, last = false;  // the seams this cell looks across
    if (ALL) {
        if (t >= a.rows * a.cols) return;
        r = t / a.cols, c = t % a.cols;
        over_row = over_col = true;
    } else {
        const int tile = t / FRONTIER_SEAM, k = t % FRONTIER_SEAM;
        if (tile >= a.tiles_x * a.tiles_y || k == FRONTIER_SEAM - 1) return;
        const int ty = tile / a.tiles_x, tx = tile % a.tiles_x;
        // k < 64: cell (0, k) of the tile; else cell (k - 63, 0)
        r = ty * FRONTIER_TILE + (k < FRONTIER_TILE ? 0 : k - (FRONTIER_TILE - 1)), c = tx * FRONTIER_TILE + (k < FRONTIER_TILE ? k : 0);
        if (r >= a.rows || c >= a.cols) return;
        over_row = k < FRONTIER_TILE, over_col = k == 0 || k >= FRONTIER_TILE;
        corner = k == 0, last = k == FRONTIER_SEAM - 2;
    }
    const int i = r * a.cols + c;
    if (agent_load(a.parent, i) < 0) return;  // no member
    int issued = 0;
    if (ALL) {
        if (c > 0) issued += seam_link(a.parent, i, i - 1);
        if (r > 0) {
            if (c > 0) issued += seam_link(a.parent, i, i - a.cols - 1);
            issued += seam_link(a.parent, i, i - a.cols);
            if (c + 1 < a.cols) issued += seam_link(a.parent, i, i - a.cols + 1);
        }
    } else {
        if (over_row && r > 0) {  // N, NW, NE over the horizontal seam; at the row's ends NW and NE lie in the diagonal tiles
            if (c > 0) issued += seam_link(a.parent, i, i - a.cols - 1);
            issued += seam_link(a.parent, i, i - a.cols);
            if (c + 1 < a.cols) issued += seam_link(a.parent, i, i - a.cols + 1);
        }
        if (over_col && c > 0) {  // W, NW, SW over the vertical seam
            issued += seam_link(a.parent, i, i - 1);
            if (!corner && r > 0) issued += seam_link(a.parent, i, i - a.cols - 1);              // the corner's NW: the row's rule has it
            if (!last && r + 1 < a.rows) issued += seam_link(a.parent, i, i + a.cols - 1);  // the last cell's SW: the NE of the tile below's first row
        }
    }
    if (COUNT && issued) atomicAdd(a.counters, (unsigned long long)issued);
}

__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_flatten(FrontierArgs a) {
    const int cells = a.rows * a.cols, i = (int)blockIdx.x * FRONTIER_THREADS + (int)threadIdx.x, lane = (int)threadIdx.x & 63;
    int lab = -1;  // also the key of a lane past the map's end: it issues nothing
    if (i < cells) {
        int x = a.parent[i];  // plain loads: parent[] was written by the launches before this one
        if (x >= 0) {
            // ends by the data alone: parents strictly descend along a chain, and nothing writes them in this launch
            for (int q = a.parent[x]; q != x; q = a.parent[x]) x = q;
            lab = x;
        }
        a.label[i] = lab;
    }
    const WaveRun run = wave_run(lab);  // every lane of the wavefront
    if (run.tail && lab >= 0) atomicAdd(a.size + lab, lane - run.head_lane + 1);
}

// A wavefront per FRONTIER_WAVE_CELLS consecutive cells: the kept roots, the roots and the members among them.
__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_count(FrontierArgs a) {
    const int cells = a.rows * a.cols, lane = (int)threadIdx.x & 63, block = (int)blockIdx.x * (FRONTIER_THREADS / 64) + ((int)threadIdx.x >> 6);
    if (block >= a.n_blocks) return;  // the whole wavefront
    int kept = 0, roots = 0, members = 0;
    for (int s = 0; s < FRONTIER_WAVE_CELLS / 64; s++) {
        const int i = block * FRONTIER_WAVE_CELLS + s * 64 + lane;
        const int lab = i < cells ? a.label[i] : -1;
        const bool root = lab == i;  // i >= 0: never for -1
        const bool keep = root && a.size[root ? i : 0] >= a.min_cells;
        kept += __popcll(__ballot(keep)), roots += __popcll(__ballot(root)), members += __popcll(__ballot(lab >= 0));
    }
    if (lane == 0) a.blocks[4 * block] = kept, a.blocks[4 * block + 1] = roots, a.blocks[4 * block + 2] = members;
}

// One workgroup: the exclusive prefix sum of the kept roots per block, and info.  A thread owns a run of consecutive blocks.
__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_scan(FrontierArgs a) {
    __shared__ int s_wave[FRONTIER_THREADS / 64];
    const int tid = (int)threadIdx.x;
    const int per = (a.n_blocks + FRONTIER_THREADS - 1) / FRONTIER_THREADS;
    const int lo = min(tid * per, a.n_blocks), hi = min(lo + per, a.n_blocks);
    int kept = 0, roots = 0, members = 0;
    for (int k = lo; k < hi; k++) kept += a.blocks[4 * k], roots += a.blocks[4 * k + 1], members += a.blocks[4 * k + 2];
    int all_kept, all_roots, all_members;  // every thread gets to the three scans
    int run = block_exclusive_scan<FRONTIER_THREADS>(kept, s_wave, &all_kept);
    block_exclusive_scan<FRONTIER_THREADS>(roots, s_wave, &all_roots);
    block_exclusive_scan<FRONTIER_THREADS>(members, s_wave, &all_members);
    for (int k = lo; k < hi; k++) {
        a.blocks[4 * k + 3] = run;
        run += a.blocks[4 * k];
    }
    if (tid == 0) a.info[0] = all_kept, a.info[1] = all_roots, a.info[2] = all_members, a.info[3] = min(all_kept, a.capacity);
}

// A kept root takes the row of its rank, if that is below capacity, and every root leaves its rank - or -1 - where its count was.
__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_rank(FrontierArgs a) {
    const int cells = a.rows * a.cols, lane = (int)threadIdx.x & 63, block = (int)blockIdx.x * (FRONTIER_THREADS / 64) + ((int)threadIdx.x >> 6);
    if (block >= a.n_blocks) return;  // the whole wavefront
    int row = a.blocks[4 * block + 3];
    for (int s = 0; s < FRONTIER_WAVE_CELLS / 64; s++) {
        const int i = block * FRONTIER_WAVE_CELLS + s * 64 + lane;
        const bool root = i < cells && a.label[i] == i;
        const int size = root ? a.size[i] : 0;
        const bool keep = root && size >= a.min_cells;
        const unsigned long long m = __ballot(keep);  // every lane of the wavefront
        const int rank = row + lanes_below(m);
        if (root) {
            const bool written = keep && rank < a.capacity;
            a.size[i] = written ? rank : -1;
            if (written) {
                int32_t *c = a.clusters + 8 * (size_t)rank;  // rep_r, rep_c stay -1 until k_frontier_reps; the box starts empty
                c[0] = i, c[1] = size, c[4] = 0x7FFFFFFF, c[5] = 0x7FFFFFFF, c[6] = -1, c[7] = -1;
            }
        }
        row += __popcll(m);
    }
}

// Every member whose root has a rank: its row and column into the sums and the box of that row.  Runs of equal ranks in consecutive
// lanes are combined first; the lanes without a rank form runs of -1 that issue nothing.
__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_stats(FrontierArgs a) {
    const int cells = a.rows * a.cols, i = (int)blockIdx.x * FRONTIER_THREADS + (int)threadIdx.x;
    int rank = -1;
    if (i < cells) {
        const int lab = a.label[i];
        if (lab >= 0) rank = a.size[lab];
    }
    const int r = i / a.cols, c = i % a.cols;
    long long sum_r = r, sum_c = c;
    int r_lo = r, r_hi = r, c_lo = c, c_hi = c;
    const WaveRun run = wave_run(rank);  // every lane of the wavefront
    wave_run_scan(run, [&](int d, bool take) {
        const long long o_sr = __shfl_up(sum_r, d, 64), o_sc = __shfl_up(sum_c, d, 64);
        const int o_rl = __shfl_up(r_lo, d, 64), o_rh = __shfl_up(r_hi, d, 64), o_cl = __shfl_up(c_lo, d, 64), o_ch = __shfl_up(c_hi, d, 64);
        if (take) sum_r += o_sr, sum_c += o_sc, r_lo = min(r_lo, o_rl), r_hi = max(r_hi, o_rh), c_lo = min(c_lo, o_cl), c_hi = max(c_hi, o_ch);
    });
    if (run.tail && rank >= 0) {
        unsigned long long *sums = reinterpret_cast<unsigned long long *>(a.sums) + 2 * (size_t)rank;
        int32_t *box = a.clusters + 8 * (size_t)rank + 4;
        atomicAdd(sums, (unsigned long long)sum_r), atomicAdd(sums + 1, (unsigned long long)sum_c);
        atomicMin(box, r_lo), atomicMin(box + 1, c_lo), atomicMax(box + 2, r_hi), atomicMax(box + 3, c_hi);
    }
}

// The representative: the least d2 << 23 | index over the members, d2 the squared distance to the integer centroid cell.
__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_keys(FrontierArgs a) {
    const int cells = a.rows * a.cols, i = (int)blockIdx.x * FRONTIER_THREADS + (int)threadIdx.x;
    int rank = -1;
    if (i < cells) {
        const int lab = a.label[i];
        if (lab >= 0) rank = a.size[lab];
    }
    unsigned long long key = ~0ull;
    if (rank >= 0) {
        const long long size = a.clusters[8 * (size_t)rank + 1], sum_r = a.sums[2 * (size_t)rank], sum_c = a.sums[2 * (size_t)rank + 1];  // complete: the launch before
        const long long dr = i / a.cols - (2 * sum_r + size) / (2 * size), dc = i % a.cols - (2 * sum_c + size) / (2 * size);
        key = (unsigned long long)(dr * dr + dc * dc) << FRONTIER_INDEX_BITS | (unsigned)i;  // d2 < 2^31, i < 2^23
    }
    const WaveRun run = wave_run(rank);  // every lane of the wavefront
    wave_run_scan(run, [&](int d, bool take) {
        const unsigned long long o = __shfl_up(key, d, 64);
        if (take) key = min(key, o);
    });
    if (run.tail && rank >= 0) atomicMin(a.key + rank, key);
}

__global__ __launch_bounds__(FRONTIER_THREADS) void k_frontier_reps(FrontierArgs a) {
    const int k = (int)blockIdx.x * FRONTIER_THREADS + (int)threadIdx.x;
    if (k >= a.capacity || a.clusters[8 * (size_t)k] < 0) return;  // no barrier in this kernel
    const int i = (int)(a.key[k] & ((1ull << FRONTIER_INDEX_BITS) - 1));
    a.clusters[8 * (size_t)k + 2] = i / a.cols, a.clusters[8 * (size_t)k + 3] = i % a.cols;
}

hipError_t launch_frontier_cells(const FrontierCellsArgs &a, hipStream_t st) {
    const int64_t cells = (int64_t)a.rows * a.cols;
    hipLaunchKernelGGL(k_frontier_cells, dim3((unsigned)((cells + FRONTIER_SPAN - 1) / FRONTIER_SPAN)), dim3(FRONTIER_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_frontier_clusters(const FrontierArgs &a, size_t size_bytes, size_t key_bytes, hipStream_t st) {
    hipError_t e = hipMemsetAsync(a.size, 0, size_bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.key, 0xFF, key_bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(a.clusters, 0xFF, (size_t)a.capacity * 8 * sizeof(int32_t), st);
    if (e == hipSuccess) e = hipMemsetAsync(a.sums, 0, (size_t)a.capacity * 2 * sizeof(long long), st);
    if (e != hipSuccess) return e;
    const int cells = a.rows * a.cols;
    const dim3 threads(FRONTIER_THREADS), per_cell((cells + FRONTIER_THREADS - 1) / FRONTIER_THREADS);
    const dim3 per_wave((a.n_blocks + FRONTIER_THREADS / 64 - 1) / (FRONTIER_THREADS / 64));
    if (a.no_tiles) {
        hipLaunchKernelGGL(k_frontier_init, per_cell, threads, 0, st, a);
        if (a.counters) hipLaunchKernelGGL((k_frontier_seams<true, true>), per_cell, threads, 0, st, a);
        else hipLaunchKernelGGL((k_frontier_seams<true, false>), per_cell, threads, 0, st, a);
    } else {
        const dim3 tiles(a.tiles_x, a.tiles_y), seams((a.tiles_x * a.tiles_y * FRONTIER_SEAM + FRONTIER_THREADS - 1) / FRONTIER_THREADS);
        if (a.counters) {
            hipLaunchKernelGGL(k_frontier_tiles<true>, tiles, threads, 0, st, a);
            hipLaunchKernelGGL((k_frontier_seams<false, true>), seams, threads, 0, st, a);
        } else {
            hipLaunchKernelGGL(k_frontier_tiles<false>, tiles, threads, 0, st, a);
            hipLaunchKernelGGL((k_frontier_seams<false, false>), seams, threads, 0, st, a);
        }
    }
    hipLaunchKernelGGL(k_frontier_flatten, per_cell, threads, 0, st, a);
    hipLaunchKernelGGL(k_frontier_count, per_wave, threads, 0, st, a);
    hipLaunchKernelGGL(k_frontier_scan, dim3(1), threads, 0, st, a);
    hipLaunchKernelGGL(k_frontier_rank, per_wave, threads, 0, st, a);
    hipLaunchKernelGGL(k_frontier_stats, per_cell, threads, 0, st, a);
    hipLaunchKernelGGL(k_frontier_keys, per_cell, threads, 0, st, a);
    hipLaunchKernelGGL(k_frontier_reps, dim3((a.capacity + FRONTIER_THREADS - 1) / FRONTIER_THREADS), threads, 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
