// The surface normals of the voxels of the world-fixed voxel map, and a frame's rows paired with their nearest voxels and reduced to the
// integers one round of point-to-plane alignment needs: include/stereo_vision_hip.h (Y), restated in stereo_vision/sv.py
// (voxel_map_normals, voxel_map_align_plane_sums).  The map's buffer is voxel_map_kernels.h's and is only read; the row's way into a cell,
// the probe's steps, the filters and a voxel's mean position are voxel_map_table.h's.  The cells around a voxel or a row are probed as
// voxel_align_kernels.hip probes them - nine side by side, an all-zero entry for a miss, so that no load waits for a branch -; that file
// keeps its own text, which its kernel's code and time depend on, and the two kernels here share probe_cells and load_entries.
//
//   normals  a lane per slot, grid slots / 256.  A member's 27 cells a plane of nine at a time; N, s1[3] and s2[6] in registers, all below
//            2^31: |e| <= 511 and N <= 27 give s2 <= 27 * 511^2, |s1| <= 27 * 511, |C_ij| < 2^28 and T < 3 * 2^28.  The table is staged
//            in LDS, VNORMAL_TILE directions at a time, as the six products d_i d_j (the mixed ones doubled) and s, which every lane
//            reads at the same address; per direction six 32 x 32 -> 64 multiply-adds and two cross-multiplied compares (Q < 2^46, s <
//            2^16: the products stay below 2^62), no division; two 64-bit divisions per voxel behind the loop.  PRUNING: a member with N
//            < min_nb gets no normal whatever the table says, so where no `fit` is asked for its search is left out - the same normal
//            and counts; VNORMAL_NO_PRUNE switches that off.  The three counts by ballot, one flush per workgroup - the only atomics.
//   score    voxel_align_kernels.hip's score kernel with 32 sums: grid (row chunk, frame), a row per lane.  Behind the search one load of
//            normal[slot] and the direction's four bytes from LDS, where the table is staged once per workgroup.
//   sums     a workgroup per frame: eight groups of 32 threads, a thread per word, add the partials of the chunks that have rows.
//
// widths   p, q < 2^28 and |origin| <= 2^30: p - o fits 32 bits, the lever arm 28; a_i = (l x nu)_i fits 37 bits, b 19; every product is
//          made in 64 bits and the sums wrap as the definition's int64 do (contract: sum w (256 |l|max)^2 < 2^63).
//
// Every load of a row is guarded by row < min(counts[b], cap), every per-row store by row < cap, every slot index is masked by slots - 1
// or is the lane's own slot < slots, a direction's index is held against K before it is used, and every LDS index is below its array's
// length: k < VNORMAL_TILE in the normals kernel, dir < K <= VNORMAL_DIRS_MAX in the score kernel.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "voxel_map_table.h"
#include "voxel_normal_kernels.h"
#include "wave_ops.h"

namespace sv {

namespace {

// What a cell without a matching key loads in place of an entry: n = 0, which no filter passes.
__device__ const unsigned long long g_no_entry[VMAP_ENTRY_WORDS] = {0ull};

// The slots of the N cells whose keys are `want` - VMAP_EMPTY for a cell that is left out - and whether each holds its key.  Every trip to
// memory is made for all N cells side by side: the first probes, then, a step at a time, the rest of the probes that began at another
// voxel's key (vmap_find's sequence, by its steps in voxel_map_table.h).  A probe that has ended stays at its slot.
template <int N>
__device__ __forceinline__ void probe_cells(const unsigned long long *table, int log2_slots, const unsigned long long (&want)[N], uint32_t (&at)[N], bool (&hit)[N]) {
    unsigned long long got[N];
#pragma unroll
    for (int h = 0; h < N; h++) {
        at[h] = want[h] != VMAP_EMPTY ? vmap_slot_of(log2_slots, want[h]) : 0u;  // < slots
        got[h] = want[h] != VMAP_EMPTY ? table[(size_t)at[h] * VMAP_ENTRY_WORDS + VMAP_KEY] : VMAP_EMPTY;
    }
    for (size_t probe = 1; probe >> log2_slots == 0; probe++) {  // after `slots` probes a full table without the key ends them
        bool more = false;
        unsigned long long next[N];
#pragma unroll
        for (int h = 0; h < N; h++) {
            const bool on = want[h] != VMAP_EMPTY && vmap_probe_goes_on(got[h], want[h]);
            at[h] = on ? vmap_next_slot(log2_slots, at[h]) : at[h];
            next[h] = table[(size_t)at[h] * VMAP_ENTRY_WORDS + VMAP_KEY];
            more = more || on;
        }
#pragma unroll
        for (int h = 0; h < N; h++) got[h] = want[h] != VMAP_EMPTY ? next[h] : VMAP_EMPTY;
        if (!more) break;
    }
#pragma unroll
    for (int h = 0; h < N; h++) hit[h] = want[h] != VMAP_EMPTY && got[h] == want[h];
}

// The words of the N entries that count - n, S, m and seq -, those of g_no_entry for a cell without a match.
template <int N>
__device__ __forceinline__ void load_entries(const unsigned long long *table, const uint32_t (&at)[N], const bool (&hit)[N], unsigned long long (&e)[N][VMAP_ENTRY_WORDS]) {
#pragma unroll
    for (int h = 0; h < N; h++) {
        const unsigned long long *in = hit[h] ? table + (size_t)at[h] * VMAP_ENTRY_WORDS : g_no_entry;
        e[h][VMAP_N] = in[VMAP_N], e[h][VMAP_M] = in[VMAP_M], e[h][VMAP_SEQ] = in[VMAP_SEQ];
#pragma unroll
        for (int k = 0; k < 3; k++) e[h][VMAP_S + k] = in[VMAP_S + k];
    }
}

// The keys of the nine cells of plane zc around (cx, cy): VMAP_EMPTY for a cell outside the box - tested BEFORE a key is formed: a cell of
// -1 shifts into the all-ones word and a cell of 2^20 carries into the next axis - and for one that `leave` names.
__device__ __forceinline__ unsigned long long cell_key_or_none(const int *nc, int xc, int yc, int zc, bool leave) {
    const bool on = (unsigned)xc < (unsigned)nc[0] && (unsigned)yc < (unsigned)nc[1] && !leave;
    return on ? vmap_key(xc, yc, zc) : VMAP_EMPTY;
}

__device__ __forceinline__ int byte_of(int32_t word, int k) { return (int)(int8_t)(word >> (8 * k)); }

// ------------------------------------------------------------------------------------------------------------------ normals

__global__ __launch_bounds__(VNORMAL_THREADS) void k_vnormal(VoxelNormalArgs a) {
    __shared__ int4 s_dir[VNORMAL_TILE][2];  // {xx, yy, zz, 2xy}, {2xz, 2yz, s, 0}
    __shared__ unsigned s_cnt[VNORMAL_THREADS / 64][3];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t slot = (size_t)blockIdx.x * VNORMAL_THREADS + (size_t)tid;  // < slots: the grid is slots / VNORMAL_THREADS
    const unsigned long long *table = vmap_table(a.map);
    const unsigned long long *own = table + slot * VMAP_ENTRY_WORDS;
    const unsigned long long key = vmap_overflowed_before(a.map) ? VMAP_EMPTY : own[VMAP_KEY];
    const bool member = key != VMAP_EMPTY && vmap_passes(a, own);  // min_n >= 1: a tombstone fails
    int N = 0, s1[3] = {0, 0, 0}, s2[6] = {0, 0, 0, 0, 0, 0};  // s2: xx, yy, zz, xy, xz, yz
    if (member) {
        int c[3], qv[3];
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = vmap_key_cell(key, k), qv[k] = vmap_zq(key, k, own[VMAP_S + k], own[VMAP_N]);
#pragma unroll 1
        for (int dz = -1; dz <= 1; dz++) {
            const int zc = c[2] + dz;
            if ((unsigned)zc >= (unsigned)a.nc[2]) continue;
            unsigned long long want[9], e[9][VMAP_ENTRY_WORDS];
            uint32_t at[9];
            bool hit[9];
#pragma unroll
            for (int h = 0; h < 9; h++) want[h] = cell_key_or_none(a.nc, c[0] + h % 3 - 1, c[1] + h / 3 - 1, zc, false);
            probe_cells<9>(table, a.log2_slots, want, at, hit);
            load_entries<9>(table, at, hit, e);
#pragma unroll
            for (int h = 0; h < 9; h++) {
                if (!hit[h] || !vmap_passes(a, e[h])) continue;  // the voxel itself is among them
                int d[3];
#pragma unroll
                for (int k = 0; k < 3; k++) d[k] = vmap_zq(want[h], k, e[h][VMAP_S + k], e[h][VMAP_N]) - qv[k], s1[k] += d[k], s2[k] += d[k] * d[k];  // |d| <= 511
                N++, s2[3] += d[0] * d[1], s2[4] += d[0] * d[2], s2[5] += d[1] * d[2];
            }
        }
    }
    // C = N s2 - s1 s1^T in the order of s2, |C_ij| < 2^28; T < 3 * 2^28
    const int C[6] = {N * s2[0] - s1[0] * s1[0], N * s2[1] - s1[1] * s1[1], N * s2[2] - s1[2] * s1[2], N * s2[3] - s1[0] * s1[1], N * s2[4] - s1[0] * s1[2], N * s2[5] - s1[1] * s1[2]};
    const int T = C[0] + C[1] + C[2];
    const bool enough = member && N >= a.min_nb;
    const bool search = member && (enough || a.fit != nullptr || (a.flags & VNORMAL_NO_PRUNE));
    long long bQ = 0, wQ = 0;
    int bs = 1, ws = 1, best = -1, worst = -1;
    for (int base = 0; base < a.K; base += VNORMAL_TILE) {
        const int cnt = a.K - base < VNORMAL_TILE ? a.K - base : (int)VNORMAL_TILE;
        __syncthreads();  // every thread of the workgroup gets here: the tile before this one has been read
        for (int k = tid; k < cnt; k += VNORMAL_THREADS) {
            const int32_t word = reinterpret_cast<const int32_t *>(a.dirs)[base + k];  // base + k < K
            const int x = byte_of(word, 0), y = byte_of(word, 1), z = byte_of(word, 2);
            s_dir[k][0] = make_int4(x * x, y * y, z * z, 2 * x * y);
            s_dir[k][1] = make_int4(2 * x * z, 2 * y * z, x * x + y * y + z * z, 0);
        }
        __syncthreads();
        if (search) {
            for (int k = 0; k < cnt; k++) {  // the same address in every lane
                const int4 u = s_dir[k][0], v = s_dir[k][1];
                const int s = v.z;
                if (s == 0) continue;  // never chosen; the same in every lane
                const long long Q = (long long)u.x * C[0] + (long long)u.y * C[1] + (long long)u.z * C[2] + (long long)u.w * C[3] + (long long)v.x * C[4] + (long long)v.y * C[5];
                const bool flatter = best < 0 || Q * bs < bQ * s;  // strict: a tie stays with the lower index
                const bool wider = worst < 0 || Q * ws > wQ * s;
                best = flatter ? base + k : best, bQ = flatter ? Q : bQ, bs = flatter ? s : bs;
                worst = wider ? base + k : worst, wQ = wider ? Q : wQ, ws = wider ? s : ws;
            }
        }
    }
    const long long lam3 = best >= 0 ? bQ / bs : 0, lam1 = worst >= 0 ? wQ / ws : 0, lam2 = (long long)T - lam1 - lam3;
    const bool given = enough && best >= 0 && lam2 > 0 && 256 * lam3 <= a.flat * lam2 && 256 * lam2 >= a.wide * lam1;
    a.normal[slot] = given ? best : -1;
    if (a.fit) {
        long long *out = a.fit + slot * 4;
        out[0] = member ? N : 0, out[1] = member ? lam1 : 0, out[2] = member ? lam2 : 0, out[3] = member ? lam3 : 0;
    }
    const unsigned long long masks[3] = {__ballot(member), __ballot(enough), __ballot(given)};  // every lane gets here
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 3; j++) s_cnt[wave][j] = (unsigned)__popcll(masks[j]);
    }
    __syncthreads();
    if (tid < 3) {
        unsigned v = 0;
#pragma unroll
        for (int w = 0; w < VNORMAL_THREADS / 64; w++) v += s_cnt[w][tid];
        if (v) atomicAdd(a.counts + tid, (unsigned long long)v);
    }
}

// ------------------------------------------------------------------------------------------------------------------ plane sums

// The nearest voxel so far of one row.
struct Nearest {
    int d2;                  // INT_MAX: none
    unsigned long long key;  // VMAP_EMPTY: none
    uint32_t slot;
    int q[3];
};

// The least d2 a voxel of the cell at offset dk from the row's own can have on one axis, squared.
__device__ __forceinline__ int axis_bound(int dk, int sub) {
    const int g = dk == 0 ? 0 : dk > 0 ? 256 - sub : sub + 1;
    return g * g;
}

// The voxels of the nine cells whose keys are `want`, each held against the nearest so far; the filters, the divisions and the comparison
// come last, for the cells whose bound the best so far has not passed meanwhile.
__device__ __forceinline__ void nearest_of(const VoxelPlaneArgs &a, const unsigned long long *table, const unsigned long long (&want)[9], const int (&bound)[9], const int *p, int far,
                                           bool skip, Nearest &best) {
    uint32_t at[9];
    bool hit[9];
    unsigned long long e[9][VMAP_ENTRY_WORDS];
    probe_cells<9>(table, a.log2_slots, want, at, hit);
    load_entries<9>(table, at, hit, e);
#pragma unroll
    for (int h = 0; h < 9; h++) {
        if (!hit[h]) continue;  // no such cell, or no voxel in it
        if (skip && bound[h] > (best.d2 < far ? best.d2 : far)) continue;  // the best may have come nearer meanwhile
        if (!vmap_passes(a, e[h])) continue;  // min_n >= 1: a tombstone fails
        int q[3], d2 = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            q[k] = vmap_zq(want[h], k, e[h][VMAP_S + k], e[h][VMAP_N]);
            d2 += (p[k] - q[k]) * (p[k] - q[k]);  // |p - q| <= 511 per axis
        }
        if (d2 < best.d2 || (d2 == best.d2 && want[h] < best.key)) best.d2 = d2, best.key = want[h], best.slot = at[h], best.q[0] = q[0], best.q[1] = q[1], best.q[2] = q[2];
    }
}

template <int DT, bool PER_ROW>
__global__ __launch_bounds__(VPLANE_THREADS) void k_vplane_score(VoxelPlaneArgs a) {
    __shared__ unsigned long long s_acc[VPLANE_THREADS / 64][VPLANE_WORDS];
    __shared__ int32_t s_nu[VNORMAL_DIRS_MAX];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (int)blockIdx.x, b = (int)blockIdx.y;
    const int cnt = vmap_rows_of(a.counts, b, a.cap);
    const int rows = vmap_overflowed_before(a.map) || cnt < 0 ? 0 : cnt;
    const int upto = PER_ROW ? a.cap : rows;  // the per-row outputs are written up to cap
    if ((long long)chunk * VPLANE_CHUNK >= upto) return;  // the whole workgroup
    for (int k = tid; k < a.K; k += VPLANE_THREADS) s_nu[k] = reinterpret_cast<const int32_t *>(a.dirs)[k];  // K <= VNORMAL_DIRS_MAX
    __syncthreads();  // every thread of the workgroup gets here
    const unsigned long long *table = vmap_table(a.map);
    const double *pose = a.poses + (size_t)b * 12;  // the same address in every lane
    const long long o[3] = {a.origin[3 * b], a.origin[3 * b + 1], a.origin[3 * b + 2]};
    const bool skip = !(a.flags & VPLANE_NO_SKIP);
    unsigned long long acc[VPLANE_WORDS];
#pragma unroll
    for (int j = 0; j < VPLANE_WORDS; j++) acc[j] = 0ull;

    for (long long tile = chunk; tile * VPLANE_CHUNK < upto; tile += a.n_chunks) {  // the same trips for every thread
        const long long i = tile * VPLANE_CHUNK + tid;
        if (i >= upto) continue;  // no shuffle and no barrier in here
        const size_t at_row = (size_t)b * a.cap + (size_t)i;
        Nearest best = {INT_MAX, VMAP_EMPTY, 0u, {0, 0, 0}};
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
                const int far = PER_ROW ? INT_MAX : a.max_d2;  // what a cell's bound is held against besides the best so far
#pragma unroll 1
                for (int zi = 0; zi < 3; zi++) {
                    const int dz = zi == 0 ? 0 : zi == 1 ? -1 : 1;  // the row's own plane first
                    const int bz = axis_bound(dz, sub[2]);
                    const int zc = c[2] + dz;
                    if ((unsigned)zc >= (unsigned)a.nc[2]) continue;
                    if (skip && bz > (best.d2 < far ? best.d2 : far)) continue;
                    unsigned long long want[9];
                    int bound[9];
#pragma unroll
                    for (int h = 0; h < 9; h++) {
                        const int dx = h % 3 - 1, dy = h / 3 - 1;
                        bound[h] = axis_bound(dx, sub[0]) + axis_bound(dy, sub[1]) + bz;
                        want[h] = cell_key_or_none(a.nc, c[0] + dx, c[1] + dy, zc, skip && bound[h] > (best.d2 < far ? best.d2 : far));
                    }
                    nearest_of(a, table, want, bound, p, far, skip, best);
                }
            }
        }
        const bool have = best.key != VMAP_EMPTY;
        const int32_t word = have ? a.normal[best.slot] : -1;  // best.slot < slots
        const int dir = word >= 0 && word < a.K ? word : -1;
        if (PER_ROW) {
            a.pair_key[at_row] = have ? (long long)best.key : -1ll;
            a.pair_d2[at_row] = have ? best.d2 : -1;
            a.pair_normal[at_row] = dir;
        }
        if (have && best.d2 <= a.max_d2) {
            acc[1] += 1ull;
            if (dir >= 0) {
                const unsigned long long w = (unsigned long long)wt;  // 1 .. 2^31 - 1
                const int32_t packed = s_nu[dir];  // dir < K
                long long nu[3], lever[3];
                int bb = 0;
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    nu[k] = byte_of(packed, k);
                    lever[k] = ((long long)p[k] - o[k]) >> VPLANE_LEVER_SHIFT;  // arithmetic: a floor
                    bb += (int)nu[k] * (best.q[k] - p[k]);
                }
                // two's complement throughout: the low 64 bits are the signed products'
                const unsigned long long av[6] = {(unsigned long long)(lever[1] * nu[2] - lever[2] * nu[1]), (unsigned long long)(lever[2] * nu[0] - lever[0] * nu[2]),
                                                  (unsigned long long)(lever[0] * nu[1] - lever[1] * nu[0]), (unsigned long long)nu[0], (unsigned long long)nu[1], (unsigned long long)nu[2]};
                const unsigned long long ub = (unsigned long long)(long long)bb, wb = w * ub;
                acc[2] += 1ull, acc[3] += w, acc[4] += wb * ub;
                int at = 11;
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    acc[5 + r] += wb * av[r];
                    const unsigned long long wa = w * av[r];
#pragma unroll
                    for (int m = r; m < 6; m++) acc[at++] += wa * av[m];
                }
            }
        }
    }
    if ((long long)chunk * VPLANE_CHUNK >= rows) return;  // the whole workgroup: no partial of a chunk without rows
#pragma unroll
    for (int j = 0; j < VPLANE_WORDS; j++) {
        const unsigned long long v = wave_sum(acc[j]);  // every lane of the workgroup gets here
        if (lane == 0) s_acc[wave][j] = v;
    }
    __syncthreads();
    if (tid < VPLANE_WORDS) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < VPLANE_THREADS / 64; w++) v += s_acc[w][tid];
        a.partials[((size_t)b * a.n_chunks + (size_t)chunk) * VPLANE_WORDS + tid] = v;
    }
}

__global__ __launch_bounds__(VPLANE_SUM_THREADS) void k_vplane_sums(VoxelPlaneArgs a) {
    __shared__ unsigned long long s_part[VPLANE_SUM_GROUPS][VPLANE_WORDS];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.x;
    const int group = tid / VPLANE_WORDS, word = tid % VPLANE_WORDS;  // a group of 32 threads takes every VPLANE_SUM_GROUPS-th chunk
    const int cnt = vmap_rows_of(a.counts, b, a.cap);
    const int rows = vmap_overflowed_before(a.map) || cnt < 0 ? 0 : cnt;
    const int tiles = (int)(((long long)rows + VPLANE_CHUNK - 1) / VPLANE_CHUNK);
    const int live = tiles < a.n_chunks ? tiles : a.n_chunks;  // the chunks whose partials were stored
    const unsigned long long *in = a.partials + (size_t)b * a.n_chunks * VPLANE_WORDS + word;
    unsigned long long v = 0;
    for (int c = group; c < live; c += VPLANE_SUM_GROUPS) v += in[(size_t)c * VPLANE_WORDS];
    s_part[group][word] = v;  // group < VPLANE_SUM_GROUPS: 256 threads are eight groups of 32
    __syncthreads();  // every thread of the workgroup gets here
    if (tid < VPLANE_WORDS) {
        unsigned long long t = 0;
#pragma unroll
        for (int g = 0; g < VPLANE_SUM_GROUPS; g++) t += s_part[g][tid];
        a.sums[(size_t)b * VPLANE_WORDS + tid] = (long long)t;
    }
}

template <int DT>
void launch_score(const VoxelPlaneArgs &a, dim3 grid, hipStream_t st) {
    if (a.pair_key) hipLaunchKernelGGL((k_vplane_score<DT, true>), grid, dim3(VPLANE_THREADS), 0, st, a);
    else hipLaunchKernelGGL((k_vplane_score<DT, false>), grid, dim3(VPLANE_THREADS), 0, st, a);
}

}  // namespace

hipError_t launch_voxel_normals(const VoxelNormalArgs &a, hipStream_t st) {
    if (hipMemsetAsync(a.counts, 0, 4 * sizeof(unsigned long long), st) != hipSuccess) return hipErrorLaunchFailure;
    const unsigned groups = (unsigned)(((size_t)1 << a.log2_slots) / VNORMAL_THREADS);  // slots >= 1024, a power of two
    hipLaunchKernelGGL(k_vnormal, dim3(groups), dim3(VNORMAL_THREADS), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_plane_align(int dtype, const VoxelPlaneArgs &a, hipStream_t st) {
    if (dtype != VMAP_F32 && dtype != VMAP_F64) return hipErrorInvalidValue;
    if (a.cap > 0) {
        const dim3 grid((unsigned)a.n_chunks, (unsigned)a.B);
        if (dtype == VMAP_F32) launch_score<VMAP_F32>(a, grid, st);
        else launch_score<VMAP_F64>(a, grid, st);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    hipLaunchKernelGGL(k_vplane_sums, dim3((unsigned)a.B), dim3(VPLANE_SUM_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
