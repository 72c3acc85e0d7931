// A frame's rows paired with their nearest voxels of the world-fixed voxel map, and the pairs reduced to the integers a closed-form
// rigid fit needs - one round of ICP: include/stereo_vision_hip.h (X), restated in stereo_vision/sv.py (voxel_map_align_sums).  The
// map's buffer is voxel_map_kernels.h's and is only read; the row's way into a cell, the probe, the filters and a voxel's mean position
// are voxel_map_table.h's.  Two kernels, no atomics, and no workgroup waits for another:
//
//   score  grid (row chunk, frame).  A lane walks VALIGN_ROWS rows of its chunk - and of the chunks n_chunks further on, for a frame of
//          more than n_chunks of them - and keeps its 19 sums in registers.  Per row: voxel_map_insert's transform in double and in its
//          order under the frame's pose, whose twelve words every lane reads from the same address (a scalar load), the cell, the offsets
//          and the position p = 256 c + (u >> 8).  Then the 27 cells around it, a plane of nine at a time, the row's own plane first.  The
//          lanes of a wavefront walk in step, so what counts is the trips to memory one after another, and every trip is made for the
//          nine cells side by side: the first probes (plain loads: a kernel boundary lies behind the insert), the further probes behind a
//          slot that holds another key, and the entry's n, S, m and seq only behind a key that matched.  A neighbour's cell is tested
//          against the box BEFORE its key is formed: a cell of -1 shifts into the all-ones word, which is VMAP_EMPTY - the probe would
//          "find" it at the first empty slot -, and a cell of 2^20 carries into the next axis.  A cell is left out where the least d2 a
//          voxel in it can have - per axis 0 for the row's own cell, 256 - sub towards +1, sub + 1 towards -1, sub = u >> 8 - exceeds
//          what still matters: the best d2 so far, and max_d2 as well where no per-row output asks for the nearest beyond it.  That
//          changes no result: d2 >= the bound > the best loses, ties included.
//          The wavefront's sums (wave_ops.h) go to the wavefront's cells of an LDS array, the four wavefronts' cells are added and stored
//          as the chunk's partial [frame][chunk][19].  Chunks beyond the frame's rows, and every chunk of an overflowed map, store no
//          partial - the sum kernel knows which they are -, but write the -1 of the per-row outputs.
//   sums   a workgroup per frame: thirteen groups of 19 threads, a thread per word, add the partials of the chunks that have rows, every
//          thirteenth chunk each, and the groups' sums are added in LDS.
//
// widths   p, q < 2^28 and |origin| <= 2^30: p - o and q - o fit 32 bits and are held in 64; a weight is below 2^31; every product is
//          made in 64 bits and the sums wrap as the definition's int64 do (contract: sum w r^2 < 2^63).  d2 <= 3 * 511^2 fits an int.
//
// Every load of a row is guarded by row < min(counts[b], cap), every per-row store by row < cap, every slot index is masked by slots - 1.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "voxel_align_kernels.h"
#include "voxel_map_table.h"
#include "wave_ops.h"

namespace sv {

namespace {

// The nearest voxel so far of one row.
struct Nearest {
    int d2;                  // INT_MAX: none
    unsigned long long key;  // VMAP_EMPTY: none
    int q[3];
};

// What a cell without a matching key loads in place of an entry: n = 0, which no filter passes.
__device__ const unsigned long long g_no_entry[VMAP_ENTRY_WORDS] = {0ull};

// The least d2 a voxel of the cell at offset dk from the row's own can have on one axis, squared.
__device__ __forceinline__ int axis_bound(int dk, int sub) {
    const int g = dk == 0 ? 0 : dk > 0 ? 256 - sub : sub + 1;
    return g * g;
}

// The voxels of the N cells whose keys are `want` - VMAP_EMPTY for a cell that is left out -, each held against the nearest so far.  Every
// trip to memory is made for all N cells side by side, so a wavefront, whose lanes go through this in step, waits for N cells as long
// as for one: the first probes; then, a step at a time, the rest of the probes that began at another voxel's key (vmap_find's sequence,
// by its steps in voxel_map_table.h); then the n, S, m and seq of the entries whose key matched, and only of those.  The filters, the
// divisions and the comparison come last, for the cells whose bound the best so far has not passed meanwhile.
template <int N>
__device__ __forceinline__ void nearest_of(const VoxelAlignArgs &a, const unsigned long long *table, const unsigned long long (&want)[N], const int (&bound)[N], const int *p,
                                           int far, bool skip, Nearest &best) {
    uint32_t at[N];
    unsigned long long got[N];
#pragma unroll
    for (int h = 0; h < N; h++) {
        at[h] = want[h] != VMAP_EMPTY ? vmap_slot_of(a.log2_slots, want[h]) : 0u;  // < slots
        got[h] = want[h] != VMAP_EMPTY ? table[(size_t)at[h] * VMAP_ENTRY_WORDS + VMAP_KEY] : VMAP_EMPTY;
    }
    for (size_t probe = 1; probe >> a.log2_slots == 0; probe++) {  // after `slots` probes a full table without the key ends them
        bool more = false;
        unsigned long long next[N];
#pragma unroll
        for (int h = 0; h < N; h++) {  // a probe that has ended stays at its slot and loads its key again: no load waits for a branch
            const bool on = want[h] != VMAP_EMPTY && vmap_probe_goes_on(got[h], want[h]);
            at[h] = on ? vmap_next_slot(a.log2_slots, at[h]) : at[h];
            next[h] = table[(size_t)at[h] * VMAP_ENTRY_WORDS + VMAP_KEY];
            more = more || on;
        }
#pragma unroll
        for (int h = 0; h < N; h++) got[h] = want[h] != VMAP_EMPTY ? next[h] : VMAP_EMPTY;
        if (!more) break;
    }
    unsigned long long e[N][VMAP_ENTRY_WORDS];  // the six words that count; a cell without a match reads g_no_entry's instead, so no load waits for a branch
#pragma unroll
    for (int h = 0; h < N; h++) {
        const unsigned long long *in = want[h] != VMAP_EMPTY && got[h] == want[h] ? table + (size_t)at[h] * VMAP_ENTRY_WORDS : g_no_entry;
        e[h][VMAP_N] = in[VMAP_N], e[h][VMAP_M] = in[VMAP_M], e[h][VMAP_SEQ] = in[VMAP_SEQ];
#pragma unroll
        for (int k = 0; k < 3; k++) e[h][VMAP_S + k] = in[VMAP_S + k];
    }
#pragma unroll
    for (int h = 0; h < N; h++) {
        if (want[h] == VMAP_EMPTY || got[h] != want[h]) continue;  // no such cell, or no voxel in it
        if (skip && bound[h] > (best.d2 < far ? best.d2 : far)) continue;  // the best may have come nearer meanwhile
        if (!vmap_passes(a, e[h])) continue;  // min_n >= 1: a tombstone fails
        int q[3], d2 = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            q[k] = vmap_zq(want[h], k, e[h][VMAP_S + k], e[h][VMAP_N]);
            d2 += (p[k] - q[k]) * (p[k] - q[k]);  // |p - q| <= 511 per axis
        }
        if (d2 < best.d2 || (d2 == best.d2 && want[h] < best.key)) best.d2 = d2, best.key = want[h], best.q[0] = q[0], best.q[1] = q[1], best.q[2] = q[2];
    }
}

template <int DT, bool PER_ROW>
__global__ __launch_bounds__(VALIGN_THREADS) void k_valign_score(VoxelAlignArgs a) {
    __shared__ unsigned long long s_acc[VALIGN_THREADS / 64][VALIGN_WORDS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (int)blockIdx.x, b = (int)blockIdx.y;
    const int cnt = vmap_rows_of(a.counts, b, a.cap);
    const int rows = vmap_overflowed_before(a.map) || cnt < 0 ? 0 : cnt;
    const int upto = PER_ROW ? a.cap : rows;  // the per-row outputs are written up to cap
    if ((long long)chunk * VALIGN_CHUNK >= upto) return;  // the whole workgroup
    const unsigned long long *table = vmap_table(a.map);
    const double *pose = a.poses + (size_t)b * 12;  // the same address in every lane
    const long long o[3] = {a.origin[3 * b], a.origin[3 * b + 1], a.origin[3 * b + 2]};
    const bool skip = !(a.flags & VALIGN_NO_SKIP);
    unsigned long long acc[VALIGN_WORDS];
#pragma unroll
    for (int j = 0; j < VALIGN_WORDS; j++) acc[j] = 0ull;

    for (long long tile = chunk; tile * VALIGN_CHUNK < upto; tile += a.n_chunks) {  // the same trips for every thread
#pragma unroll 1
        for (int r = 0; r < VALIGN_ROWS; r++) {
            const long long i = tile * VALIGN_CHUNK + r * VALIGN_THREADS + tid;
            if (i >= upto) continue;  // no shuffle and no barrier in here
            const size_t at_row = (size_t)b * a.cap + (size_t)i;
            Nearest best = {INT_MAX, VMAP_EMPTY, {0, 0, 0}};
            bool keep = false;
            int wt = 0, p[3] = {0, 0, 0};
            if (i < rows) {
                double x, y, z;
                vmap_load_row<DT>(a.xyz, at_row, x, y, z);
                wt = a.weight ? a.weight[at_row] : 1;
                keep = wt > 0;
                int c[3], sub[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    double t;
                    long long cell;
                    keep = vmap_cell(a, pose, k, x, y, z, keep, t, cell);
                    c[k] = (int)cell;
                    sub[k] = (int)(vmap_offset(t, cell) >> 8);
                    p[k] = c[k] * 256 + sub[k];
                }
                if (keep) {
                    acc[0] += 1ull;
                    // what a cell's bound is held against: the best so far, and max_d2 where nobody asks for the nearest beyond it
                    const int far = PER_ROW ? INT_MAX : a.max_d2;
#pragma unroll 1
                    for (int zi = 0; zi < 3; zi++) {
                        const int dz = zi == 0 ? 0 : zi == 1 ? -1 : 1;  // the row's own plane first, its own cell in it: the best comes near early
                        const int bz = axis_bound(dz, sub[2]);
                        const int zc = c[2] + dz;
                        if ((unsigned)zc >= (unsigned)a.nc[2]) continue;
                        if (skip && bz > (best.d2 < far ? best.d2 : far)) continue;
                        unsigned long long want[9];
                        int bound[9];
#pragma unroll
                        for (int h = 0; h < 9; h++) {
                            const int dx = h % 3 - 1, dy = h / 3 - 1;
                            const int xc = c[0] + dx, yc = c[1] + dy;
                            bound[h] = axis_bound(dx, sub[0]) + axis_bound(dy, sub[1]) + bz;
                            const bool on = (unsigned)xc < (unsigned)a.nc[0] && (unsigned)yc < (unsigned)a.nc[1] && !(skip && bound[h] > (best.d2 < far ? best.d2 : far));
                            want[h] = on ? vmap_key(xc, yc, zc) : VMAP_EMPTY;  // a key only of cells inside the box
                        }
                        nearest_of<9>(a, table, want, bound, p, far, skip, best);
                    }
                }
            }
            const bool have = best.key != VMAP_EMPTY;
            if (PER_ROW) {
                a.pair_key[at_row] = have ? (long long)best.key : -1ll;
                a.pair_d2[at_row] = have ? best.d2 : -1;
            }
            if (have && best.d2 <= a.max_d2) {
                const unsigned long long w = (unsigned long long)wt;  // 1 .. 2^31 - 1
                unsigned long long dp[3], dq[3];
#pragma unroll
                for (int k = 0; k < 3; k++) dp[k] = (unsigned long long)((long long)p[k] - o[k]), dq[k] = (unsigned long long)((long long)best.q[k] - o[k]);
                acc[1] += 1ull, acc[2] += w, acc[3] += w * (unsigned long long)best.d2;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const unsigned long long wp = w * dp[k];  // two's complement: the low 64 bits are the signed product's
                    acc[4 + k] += wp, acc[7 + k] += w * dq[k];
#pragma unroll
                    for (int m = 0; m < 3; m++) acc[10 + 3 * k + m] += wp * dq[m];
                }
            }
        }
    }
    if ((long long)chunk * VALIGN_CHUNK >= rows) return;  // the whole workgroup: no partial of a chunk without rows
#pragma unroll
    for (int j = 0; j < VALIGN_WORDS; j++) {
        const unsigned long long v = wave_sum(acc[j]);  // every lane of the workgroup gets here
        if (lane == 0) s_acc[wave][j] = v;
    }
    __syncthreads();
    if (tid < VALIGN_WORDS) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < VALIGN_THREADS / 64; w++) v += s_acc[w][tid];
        a.partials[((size_t)b * a.n_chunks + (size_t)chunk) * VALIGN_WORDS + tid] = v;
    }
}

__global__ __launch_bounds__(VALIGN_SUM_THREADS) void k_valign_sums(VoxelAlignArgs a) {
    __shared__ unsigned long long s_part[VALIGN_SUM_GROUPS][VALIGN_WORDS];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int group = tid / VALIGN_WORDS, word = tid % VALIGN_WORDS;  // a group of 19 threads takes every VALIGN_SUM_GROUPS-th chunk
    const int cnt = vmap_rows_of(a.counts, b, a.cap);
    const int rows = vmap_overflowed_before(a.map) || cnt < 0 ? 0 : cnt;
    const int tiles = (int)(((long long)rows + VALIGN_CHUNK - 1) / VALIGN_CHUNK);
    const int live = tiles < a.n_chunks ? tiles : a.n_chunks;  // the chunks whose partials were stored
    if (group < VALIGN_SUM_GROUPS) {
        const unsigned long long *in = a.partials + (size_t)b * a.n_chunks * VALIGN_WORDS + word;
        unsigned long long v = 0;
        for (int c = group; c < live; c += VALIGN_SUM_GROUPS) v += in[(size_t)c * VALIGN_WORDS];
        s_part[group][word] = v;
    }
    __syncthreads();  // every thread of the workgroup gets here
    if (tid < VALIGN_WORDS) {
        unsigned long long v = 0;
#pragma unroll
        for (int g = 0; g < VALIGN_SUM_GROUPS; g++) v += s_part[g][tid];
        a.sums[(size_t)b * VALIGN_WORDS + tid] = (long long)v;
    }
}

template <int DT>
void launch_score(const VoxelAlignArgs &a, dim3 grid, hipStream_t st) {
    if (a.pair_key) hipLaunchKernelGGL((k_valign_score<DT, true>), grid, dim3(VALIGN_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_valign_score<DT, false>), grid, dim3(VALIGN_THREADS), 0, st, a);
}

}  // namespace

hipError_t launch_voxel_align(int dtype, const VoxelAlignArgs &a, hipStream_t st) {
    if (dtype != VMAP_F32 && dtype != VMAP_F64) return hipErrorInvalidValue;
    if (a.cap > 0) {
        const dim3 grid((unsigned)a.n_chunks, (unsigned)a.B);
        if (dtype == VMAP_F32) launch_score<VMAP_F32>(a, grid, st);
        else launch_score<VMAP_F64>(a, grid, st);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    hipLaunchKernelGGL(k_valign_sums, dim3((unsigned)a.B), dim3(VALIGN_SUM_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
