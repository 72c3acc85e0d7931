// The connected components of a world-fixed voxel map: include/stereo_vision_hip.h (W), restated in stereo_vision/sv.py
// (voxel_map_clusters).  Integers behind the flat cell of mode 1.  The voxel map's buffer is voxel_map_kernels.h's; its filters, centre,
// height, probe and head are voxel_map_table.h's, the flat map's cell rule is occupancy_map_cells.h's.  A component is found as the
// union-find tree over the SLOTS of its members - a parent is a slot with a smaller index, the root the least slot -, which depends on
// where the inserts left the entries; what leaves this file does not: a component's identity is the least KEY of its members, and every
// statistic is a count, a sum, a minimum or a maximum of integers - the same bits whatever order the unions and the atomics take.  Only
// the order of the rows, and which kept components fall past `capacity`, follow the roots' slots; the caller sorts by least key.
//
// Eight kernels in stream order:
//
//   init     a strided walk of the table, a lane per slot and trip: parent[slot] = slot for a member - a key, the three filters, the
//            height band over z_ref_q or over the floor of the flat cell under the centre -, -1 otherwise; count[slot] = 0.  The first
//            lanes of the grid clear the rows and info.  An overflowed map has no member, and info[0] = -1.
//
//   link     the same walk.  A member forms the keys of its enabled half-neighbours - the 13, 9 or 3 offsets that are negative in (dz,
//            dy, dx) order, each tested against the box per axis BEFORE a key is made of it: key - 1 of cell (0, y, z) is the valid key
//            of another cell -, issues the first probe load of all of them together, and only then consumes them: a hit at the first
//            slot, an empty slot, or - a collision - the table's probe (vmap_find).  Plain loads of the table: no kernel writes a key
//            here.  Where the found slot is a member the two slots are united: the larger root is hooked under the smaller.
//
//            THIS IS THE ONLY LAUNCH IN WHICH A WORKGROUP READS A WORD THAT ANOTHER WORKGROUP MAY WRITE IN THE SAME LAUNCH.  In it every
//            access to parent[] is a relaxed agent-scope atomic (__hip_atomic_load / __hip_atomic_fetch_min with
//            __HIP_MEMORY_SCOPE_AGENT): a plain load could be served by the CU's L1 or the XCD's L2, which are not coherent for it.
//            There is no cooperative launch, no grid barrier, no flag, and no loop that waits for a value another thread has yet to
//            write: a thread only ever reacts to what it has read, and whatever it reads lets it go on.
//
//            Termination.  parent[] changes by fetch_min only, and only ever to a slot index that is smaller than the word's own index:
//            a root r is hooked under b < r, and the path compression at the end of a member's links lowers parent[x] to an ancestor of x, which is below x.  So
//            (1) along any chain the indices strictly descend, whatever other threads lower meanwhile, and a find ends at a word that
//            holds its own index after at most `slots` steps; (2) a unite comes round again only when its fetch_min found the word
//            already lowered by someone else (old != a) - each such event is paid for by one of the finitely many lowerings the table
//            admits: a word of parent[] can only go down and never below 0.  No loop depends on anything but the data it has read.
//
//   roots    a launch of its own: root = find(slot) by plain loads - parent[] was written by the launches before -, kept in label[slot],
//            and the members counted at count[root].  Equal roots of a wavefront are combined first (below).
//
//   count, scan, rank   the ordered compaction of the kept roots (label == own slot, size >= min_voxels), as the compact clouds and the
//            frontier do it: a wavefront owns 1024 consecutive slots, counts by ballots, one workgroup scans the counts, and the rank
//            kernel gives a kept root the row of its rank - started if the rank is below `capacity` - and leaves in count[root] the row,
//            -3 for a kept root past `capacity`, -2 for a root below min_voxels.  count also adds up info.
//
//   stats    the walk again: a member whose root has a row adds its words into that row - 64-bit integer add, min and max, none with a
//            returned value.  Equal rows of a wavefront are combined first.
//
//   resolve  the walk again: label[slot] = count[root], or -1; with `drop` a member of a component below min_voxels is emptied
//            (vmap_clear_values: the key stays, a tombstone).  The emptied voxels go by ballot, one add per workgroup.
//
// Combining equal destinations over a wavefront (roots, stats).  Neighbouring slots are hash-random, so runs of equal roots in
// consecutive lanes (wave_run) are rare, while a street's obstacle voxels are often ONE component: every lane of every wavefront would
// add to the same word.  So: the first live lane's destination is broadcast, the live lanes that share it are balloted, their payloads
// are reduced over the wavefront (wave_ops.h; the other lanes pass the neutral values to the same calls), one lane issues the atomics,
// the sharing lanes retire.  Each trip retires at least one lane: at most 64 trips.  A trip of one lane skips the reductions - the
// ballot is the same in every lane, so the branch is uniform.  What "one lane issues" means: the combined payload stays with the
// wavefront - the same words in every lane - as long as the next trips name the same destination, and goes out when another
// destination comes or the walk ends; there the four wavefronts of the workgroup meet in LDS and equal destinations go out once.  On
// the one-component map that is one set of atomics per workgroup instead of one per wavefront and trip.
//
// Every other exchange between workgroups happens across a launch boundary.  No shuffle runs under divergence and no barrier sits in a
// branch that some thread of the workgroup skips.
//
// Bounds: a slot index is < slots (the walk) or masked by slots - 1 (the probe); a neighbour's key is formed from cells inside the box
// only; a row index is < capacity (rank gives no other); a flat cell comes from map_cell, which admits (r, c) inside rows x cols only;
// parent[], count[] and label[] are indexed by slots, and by roots, which are slots; blocks[] by a wavefront's block < slots / 1024.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_cluster_kernels.h"
#include "voxel_map_table.h"
#include "wave_ops.h"

namespace sv {

namespace {

enum { VCL_MEMBERS = 0, VCL_COMPONENTS = 1, VCL_KEPT = 2, VCL_SMALL = 3, VCL_EMPTIED = 4, VCL_LARGEST = 5 };
enum { VCL_ROW_KEY = 0, VCL_ROW_VOXELS = 1, VCL_ROW_N = 2, VCL_ROW_CMIN = 3, VCL_ROW_CMAX = 6, VCL_ROW_SUM = 9, VCL_ROW_FIRST = 12, VCL_ROW_LAST = 13, VCL_ROW_M = 14 };
constexpr long long VCL_MOST = 0x7FFFFFFFFFFFFFFFll;
constexpr int VCL_SMALL_ROOT = -2, VCL_CUT_ROOT = -3;

#define VCL_WALK(slot, slots) \
    for (size_t slot = (size_t)blockIdx.x * VCLUSTER_THREADS + threadIdx.x; slot < (slots); slot += (size_t)gridDim.x * VCLUSTER_THREADS)  // the same trips for a workgroup

// ---- the union-find in global memory: relaxed agent-scope atomics only (frontier_kernels.hip holds the same three for the flat map) ----

__device__ __forceinline__ int agent_load(const int32_t *p, int x) { return __hip_atomic_load(p + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Ends by the data alone: parents strictly descend along a chain, whatever other threads lower meanwhile.
__device__ __forceinline__ int agent_find(const int32_t *p, int x) {
    for (;;) {
        const int q = agent_load(p, x);
        if (q == x) return x;
        x = q;
    }
}

// Hooks the larger root under the smaller; returns the smaller, an ancestor of both a and b from then on - a start for the caller's
// next find that is nearer the root than a was.  Ends by the data alone: a retry follows only a fetch_min that found its word lowered by
// another thread, which can happen only finitely often - every lowering takes a word of parent[] strictly down, and none goes below 0.
__device__ __forceinline__ int agent_unite(int32_t *p, int a, int b) {
    for (;;) {
        a = agent_find(p, a), b = agent_find(p, b);
        if (a == b) return a;
        if (a < b) {
            const int t = a;
            a = b, b = t;
        }
        const int old = __hip_atomic_fetch_min(p + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return b;
        a = old;
    }
}

// 64-bit integer atomics without a returned value.
__device__ __forceinline__ void row_add(long long *p, long long v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void row_min(long long *p, long long v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void row_max(long long *p, long long v) { __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Whether the entry e with the key `key` (not VMAP_EMPTY) is a member.
__device__ __forceinline__ bool vcl_member(const VoxelClusterArgs &a, unsigned long long key, const unsigned long long *e) {
    if (!vmap_passes(a, e)) return false;
    const unsigned long long n = e[VMAP_N];  // >= min_n >= 1
    long long base = a.z_ref_q;
    if (a.mode == 1) {
        const double X = vmap_centre(a.lo[0], a.size, key, 0, e[VMAP_S], n), Y = vmap_centre(a.lo[1], a.size, key, 1, e[VMAP_S + 1], n);
        int r, c;
        if (!map_cell(a.m, map_grid(a.m, X), map_grid(a.m, Y), r, c)) return false;
        base = a.floor[(size_t)r * a.m.cols + c];  // < rows * cols
        if (base == -1) return false;
    }
    const long long h = (long long)vmap_zq(key, 2, e[VMAP_S + 2], n) - base;  // 64 bits: a floor may hold any word
    return a.h_lo_q <= h && h < a.h_hi_q;
}

__global__ __launch_bounds__(VCLUSTER_THREADS) void k_vcluster_init(VoxelClusterArgs a) {
    const bool lost = vmap_overflowed_before(a.map);
    const unsigned long long *table = vmap_table(a.map);
    const size_t slots = (size_t)1 << a.log2_slots;
    const size_t words = (size_t)a.capacity * VCLUSTER_ROW_WORDS, step = (size_t)gridDim.x * VCLUSTER_THREADS;
    for (size_t i = (size_t)blockIdx.x * VCLUSTER_THREADS + threadIdx.x; i < words + VCLUSTER_INFO; i += step) {
        if (i < words) a.clusters[i] = 0ll;
        else a.info[i - words] = i - words == VCL_MEMBERS && lost ? -1ll : 0ll;
    }
    VCL_WALK(slot, slots) {
        const unsigned long long *e = table + slot * VMAP_ENTRY_WORDS;
        const unsigned long long key = e[VMAP_KEY];
        const bool member = !lost && key != VMAP_EMPTY && vcl_member(a, key, e);
        a.parent[slot] = member ? (int32_t)slot : -1;
        a.count[slot] = 0;
    }
}

// The offset o = 0 .. 12 of the half neighbourhood: the cells before the centre in (dz, dy, dx) order.
__device__ __forceinline__ void vcl_offset(int o, int &dx, int &dy, int &dz) { dz = o / 9 - 1, dy = (o / 3) % 3 - 1, dx = o % 3 - 1; }

__global__ __launch_bounds__(VCLUSTER_THREADS) void k_vcluster_link(VoxelClusterArgs a) {
    const unsigned long long *table = vmap_table(a.map);
    const size_t slots = (size_t)1 << a.log2_slots;
    const int most = a.connectivity == 6 ? 1 : a.connectivity == 18 ? 2 : 3;  // axes a neighbour may differ on
    VCL_WALK(slot, slots) {
        const int i = (int)slot;
        if (agent_load(a.parent, i) < 0) continue;  // no member; no barrier and no shuffle in this kernel
        const unsigned long long key = table[slot * VMAP_ENTRY_WORDS + VMAP_KEY];
        const int cx = vmap_key_cell(key, 0), cy = vmap_key_cell(key, 1), cz = vmap_key_cell(key, 2);
        unsigned long long want[13], got[13];
        uint32_t at[13];
#pragma unroll
        for (int o = 0; o < 13; o++) {  // the first probe of every neighbour, in flight together
            int dx, dy, dz;
            vcl_offset(o, dx, dy, dz);
            const int x = cx + dx, y = cy + dy, z = cz + dz;
            const bool on = (dx != 0) + (dy != 0) + (dz != 0) <= most && (unsigned)x < (unsigned)a.nc[0] && (unsigned)y < (unsigned)a.nc[1] && (unsigned)z < (unsigned)a.nc[2];
            want[o] = on ? vmap_key(x, y, z) : VMAP_EMPTY;  // a key only of cells inside the box
            at[o] = on ? vmap_slot_of(a.log2_slots, want[o]) : 0u;  // < slots
            got[o] = on ? table[(size_t)at[o] * VMAP_ENTRY_WORDS + VMAP_KEY] : VMAP_EMPTY;
        }
        int up = i;  // an ancestor of i, or i: where the next find for i starts
#pragma unroll
        for (int o = 0; o < 13; o++) {
            if (want[o] == VMAP_EMPTY || got[o] == VMAP_EMPTY) continue;  // no such cell, or no voxel in it
            const long long j = got[o] == want[o] ? (long long)at[o] : vmap_find(table, a.log2_slots, want[o]);  // a collision: the whole probe
            if (j < 0) continue;
            const int pj = agent_load(a.parent, (int)j);  // -1 for no member, else j or an ancestor of j: the find for j starts there
            if (pj >= 0 && pj != up) up = agent_unite(a.parent, up, pj);  // pj == up: a common ancestor, one component already
        }
        // parent[i] to an ancestor of i - below i, so chains still descend -: the roots kernel and the other lanes' finds get there in one step
        if (!(a.flags & VCLUSTER_NO_COMPRESS) && up < i) __hip_atomic_fetch_min(a.parent + i, up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(VCLUSTER_THREADS) void k_vcluster_roots(VoxelClusterArgs a) {
    __shared__ int s_root[VCLUSTER_THREADS / 64], s_members[VCLUSTER_THREADS / 64];
    const size_t slots = (size_t)1 << a.log2_slots;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int held = -1, members = 0;  // the same in every lane: the root this wavefront holds members for, over its trips, and how many
    VCL_WALK(slot, slots) {
        int x = a.parent[slot];  // plain loads: parent[] was written by the launches before this one
        if (x >= 0)              // ends by the data alone: parents strictly descend along a chain, and nothing writes them in this launch
            for (int q = a.parent[x]; q != x; q = a.parent[x]) x = q;
        a.label[slot] = x;
        if (a.flags & VCLUSTER_NO_COMBINE) {
            if (x >= 0) atomicAdd(a.count + x, 1);
            continue;
        }
        unsigned long long live = __ballot(x >= 0);  // every lane of the wavefront gets here: the walk's trips are a workgroup's
        while (live) {                               // at most 64 trips: each retires its leader at least
            const int leader = __ffsll((long long)live) - 1;
            const int r = __shfl(x, leader, 64);
            const unsigned long long same = __ballot(x == r) & live;
            if (r != held) {  // uniform
                if (lane == 0 && held >= 0) atomicAdd(a.count + held, members);
                held = r, members = 0;
            }
            members += __popcll(same);
            live &= ~same;
        }
    }
    // what the wavefronts still hold: equal roots of the workgroup in one add
    if (lane == 0) s_root[wave] = held, s_members[wave] = members;
    __syncthreads();  // every thread of the workgroup gets here
    if (threadIdx.x != 0) return;
    for (int w = 0; w < VCLUSTER_THREADS / 64; w++) {
        if (s_root[w] < 0) continue;
        int total = s_members[w];
        for (int v = w + 1; v < VCLUSTER_THREADS / 64; v++)
            if (s_root[v] == s_root[w]) total += s_members[v], s_root[v] = -1;
        atomicAdd(a.count + s_root[w], total);
    }
}

// A wavefront per VCLUSTER_WAVE_SLOTS consecutive slots: its kept roots into blocks[], and its share of info.
__global__ __launch_bounds__(VCLUSTER_THREADS) void k_vcluster_count(VoxelClusterArgs a) {
    const int lane = (int)threadIdx.x & 63, block = (int)blockIdx.x * (VCLUSTER_THREADS / 64) + ((int)threadIdx.x >> 6);
    const int n_blocks = (int)(((size_t)1 << a.log2_slots) / VCLUSTER_WAVE_SLOTS);
    if (block >= n_blocks) return;  // the whole wavefront
    int kept = 0, roots = 0, members = 0, largest = 0;
    long long small = 0;
    for (int s = 0; s < VCLUSTER_WAVE_SLOTS / 64; s++) {
        const int i = block * VCLUSTER_WAVE_SLOTS + s * 64 + lane;  // < slots
        const int lab = a.label[i];
        const bool root = lab == i;  // never for -1
        const int size = root ? a.count[i] : 0;
        const bool keep = root && size >= a.min_voxels;
        kept += __popcll(__ballot(keep)), roots += __popcll(__ballot(root)), members += __popcll(__ballot(lab >= 0));
        small += root && !keep ? size : 0;
        largest = max(largest, size);
    }
    small = wave_sum(small), largest = wave_max(largest);  // every lane of the wavefront
    if (lane != 0) return;
    a.blocks[2 * block] = kept;
    if (members) row_add(a.info + VCL_MEMBERS, members);
    if (roots) row_add(a.info + VCL_COMPONENTS, roots);
    if (kept) row_add(a.info + VCL_KEPT, kept);
    if (small) row_add(a.info + VCL_SMALL, small);
    if (largest) row_max(a.info + VCL_LARGEST, largest);
}

// One workgroup: the exclusive prefix sum of the kept roots per block.  A thread owns a run of consecutive blocks.
__global__ __launch_bounds__(VCLUSTER_THREADS) void k_vcluster_scan(VoxelClusterArgs a) {
    __shared__ int s_wave[VCLUSTER_THREADS / 64];
    const int n_blocks = (int)(((size_t)1 << a.log2_slots) / VCLUSTER_WAVE_SLOTS);
    const int tid = (int)threadIdx.x;
    const int per = (n_blocks + VCLUSTER_THREADS - 1) / VCLUSTER_THREADS;
    const int lo = min(tid * per, n_blocks), hi = min(lo + per, n_blocks);
    int kept = 0;
    for (int k = lo; k < hi; k++) kept += a.blocks[2 * k];
    int all_kept;  // every thread gets to the scan
    int run = block_exclusive_scan<VCLUSTER_THREADS>(kept, s_wave, &all_kept);
    for (int k = lo; k < hi; k++) {
        a.blocks[2 * k + 1] = run;
        run += a.blocks[2 * k];
    }
}

// A kept root takes the row of its rank, if that is below capacity, and every root leaves its row, -2 or -3 where its count was.
__global__ __launch_bounds__(VCLUSTER_THREADS) void k_vcluster_rank(VoxelClusterArgs a) {
    const int lane = (int)threadIdx.x & 63, block = (int)blockIdx.x * (VCLUSTER_THREADS / 64) + ((int)threadIdx.x >> 6);
    const int n_blocks = (int)(((size_t)1 << a.log2_slots) / VCLUSTER_WAVE_SLOTS);
    if (block >= n_blocks) return;  // the whole wavefront
    int row = a.blocks[2 * block + 1];
    for (int s = 0; s < VCLUSTER_WAVE_SLOTS / 64; s++) {
        const int i = block * VCLUSTER_WAVE_SLOTS + s * 64 + lane;
        const bool root = a.label[i] == i;
        const int size = root ? a.count[i] : 0;
        const bool keep = root && size >= a.min_voxels;
        const unsigned long long m = __ballot(keep);  // every lane of the wavefront
        const int rank = row + lanes_below(m);
        if (root) {
            const bool written = keep && rank < a.capacity;
            a.count[i] = written ? rank : keep ? VCL_CUT_ROOT : VCL_SMALL_ROOT;
            if (written) {
                long long *c = a.clusters + (size_t)rank * VCLUSTER_ROW_WORDS;  // the sums stay 0 from init
                c[VCL_ROW_KEY] = VCL_MOST, c[VCL_ROW_VOXELS] = size, c[VCL_ROW_FIRST] = VCL_MOST, c[VCL_ROW_LAST] = -1;
#pragma unroll
                for (int k = 0; k < 3; k++) c[VCL_ROW_CMIN + k] = VCL_MOST, c[VCL_ROW_CMAX + k] = -1;
            }
        }
        row += __popcll(m);
    }
}

// What a member adds to its row.
struct VclPayload {
    long long key, n, m, sum[3];
    int cmin[3], cmax[3];
    long long first, last;
};

__device__ __forceinline__ void vcl_neutral(VclPayload &p) {
    p.key = VCL_MOST, p.n = 0, p.m = 0, p.first = VCL_MOST, p.last = -1;
#pragma unroll
    for (int k = 0; k < 3; k++) p.sum[k] = 0, p.cmin[k] = 0x7FFFFFFF, p.cmax[k] = -1;
}

__device__ __forceinline__ void vcl_merge(VclPayload &p, const VclPayload &q) {
    p.key = q.key < p.key ? q.key : p.key, p.n += q.n, p.m += q.m, p.first = q.first < p.first ? q.first : p.first, p.last = q.last > p.last ? q.last : p.last;
#pragma unroll
    for (int k = 0; k < 3; k++) p.sum[k] += q.sum[k], p.cmin[k] = min(p.cmin[k], q.cmin[k]), p.cmax[k] = max(p.cmax[k], q.cmax[k]);
}

__device__ __forceinline__ void vcl_issue(long long *c, const VclPayload &p) {
    row_min(c + VCL_ROW_KEY, p.key), row_add(c + VCL_ROW_N, p.n), row_add(c + VCL_ROW_M, p.m);
#pragma unroll
    for (int k = 0; k < 3; k++) row_min(c + VCL_ROW_CMIN + k, p.cmin[k]), row_max(c + VCL_ROW_CMAX + k, p.cmax[k]), row_add(c + VCL_ROW_SUM + k, p.sum[k]);
    row_min(c + VCL_ROW_FIRST, p.first), row_max(c + VCL_ROW_LAST, p.last);
}

__global__ __launch_bounds__(VCLUSTER_THREADS) void k_vcluster_stats(VoxelClusterArgs a) {
    __shared__ int s_row[VCLUSTER_THREADS / 64];
    __shared__ VclPayload s_held[VCLUSTER_THREADS / 64];
    const unsigned long long *table = vmap_table(a.map);
    const size_t slots = (size_t)1 << a.log2_slots;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    int held_row = -1;  // the same in every lane: the row this wavefront holds a payload for, over its trips
    VclPayload held;
    vcl_neutral(held);
    VCL_WALK(slot, slots) {
        const int root = a.label[slot];
        const int row = root >= 0 ? a.count[root] : -1;  // < capacity
        VclPayload p;
        vcl_neutral(p);
        if (row >= 0) {
            const unsigned long long *e = table + slot * VMAP_ENTRY_WORDS;
            const unsigned long long key = e[VMAP_KEY], n = e[VMAP_N];  // a member: n >= 1
            p.key = (long long)key, p.n = (long long)n, p.m = (long long)e[VMAP_M];
            p.first = vmap_first_seq(e[VMAP_SEQ]), p.last = vmap_last_seq(e[VMAP_SEQ]);
#pragma unroll
            for (int k = 0; k < 3; k++) p.cmin[k] = p.cmax[k] = vmap_key_cell(key, k), p.sum[k] = vmap_zq(key, k, e[VMAP_S + k], n);
        }
        if (a.flags & VCLUSTER_NO_COMBINE) {
            if (row >= 0) vcl_issue(a.clusters + (size_t)row * VCLUSTER_ROW_WORDS, p);
            continue;
        }
        unsigned long long live = __ballot(row >= 0);  // every lane of the wavefront gets here
        while (live) {                                 // at most 64 trips
            const int leader = __ffsll((long long)live) - 1;
            const int r = __shfl(row, leader, 64);
            const unsigned long long same = __ballot(row == r) & live;
            if (__popcll(same) == 1 && r != held_row) {  // uniform: `same`, r and held_row are the same in every lane
                if (lane == leader) vcl_issue(a.clusters + (size_t)r * VCLUSTER_ROW_WORDS, p);
            } else {
                const bool in = (same >> lane) & 1;
                VclPayload q;  // of the sharing lanes; every lane calls every reduction, the others with the neutral values
                q.key = wave_min(in ? p.key : VCL_MOST), q.n = wave_sum(in ? p.n : 0ll), q.m = wave_sum(in ? p.m : 0ll);
                q.first = wave_min(in ? p.first : VCL_MOST), q.last = wave_max(in ? p.last : -1ll);
#pragma unroll
                for (int k = 0; k < 3; k++)
                    q.cmin[k] = wave_min(in ? p.cmin[k] : 0x7FFFFFFF), q.cmax[k] = wave_max(in ? p.cmax[k] : -1), q.sum[k] = wave_sum(in ? p.sum[k] : 0ll);
                if (r != held_row) {  // the reductions left q in every lane: what the wavefront holds stays uniform
                    if (lane == 0 && held_row >= 0) vcl_issue(a.clusters + (size_t)held_row * VCLUSTER_ROW_WORDS, held);
                    held_row = r;
                    vcl_neutral(held);
                }
                vcl_merge(held, q);
            }
            live &= ~same;
        }
    }
    // what the wavefronts still hold: equal rows of the workgroup in one set of atomics
    if (lane == 0) s_row[wave] = held_row, s_held[wave] = held;
    __syncthreads();  // every thread of the workgroup gets here
    if (threadIdx.x != 0) return;
    for (int w = 0; w < VCLUSTER_THREADS / 64; w++) {
        if (s_row[w] < 0) continue;
        VclPayload all = s_held[w];
        for (int v = w + 1; v < VCLUSTER_THREADS / 64; v++)
            if (s_row[v] == s_row[w]) vcl_merge(all, s_held[v]), s_row[v] = -1;
        vcl_issue(a.clusters + (size_t)s_row[w] * VCLUSTER_ROW_WORDS, all);
    }
}

__global__ __launch_bounds__(VCLUSTER_THREADS) void k_vcluster_resolve(VoxelClusterArgs a) {
    __shared__ uint32_t s_count[VCLUSTER_THREADS / 64];
    unsigned long long *table = vmap_table(a.map);
    const size_t slots = (size_t)1 << a.log2_slots;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    uint32_t emptied = 0;  // of this wavefront, over its trips
    VCL_WALK(slot, slots) {
        const int root = a.label[slot];  // this lane's own word: nobody else reads it here
        const int lab = root >= 0 ? a.count[root] : -1;
        a.label[slot] = lab;
        const bool gone = a.drop && lab == VCL_SMALL_ROOT;
        if (gone) vmap_clear_values(table + slot * VMAP_ENTRY_WORDS);
        emptied += (uint32_t)__popcll(__ballot(gone));  // every lane of the wavefront gets here
    }
    if (lane == 0) s_count[wave] = emptied;
    __syncthreads();  // every thread of the workgroup gets here
    if (threadIdx.x != 0) return;
    uint32_t total = 0;
    for (int w = 0; w < VCLUSTER_THREADS / 64; w++) total += s_count[w];
    if (total) row_add(a.info + VCL_EMPTIED, (long long)total);
}

}  // namespace

hipError_t launch_voxel_clusters(const VoxelClusterArgs &a, int max_groups, int stages, hipStream_t st) {
    if (max_groups < 1 || max_groups > VCLUSTER_MAX_GROUPS || stages < 0 || stages >= VCLUSTER_STAGES) return hipErrorInvalidValue;
    const size_t slots = (size_t)1 << a.log2_slots, tiles = slots / VCLUSTER_THREADS;  // slots is a multiple of 1024
    const dim3 walk((unsigned)(tiles < (size_t)max_groups ? tiles : (size_t)max_groups)), threads(VCLUSTER_THREADS);
    const dim3 waves((unsigned)((slots / VCLUSTER_WAVE_SLOTS + VCLUSTER_THREADS / 64 - 1) / (VCLUSTER_THREADS / 64)));
    int k = 0;
#define VCL_LAUNCH(kernel, grid)                                            \
    hipLaunchKernelGGL(kernel, grid, threads, 0, st, a);                    \
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;      \
    if (++k == stages) return hipSuccess;
    VCL_LAUNCH(k_vcluster_init, walk)
    VCL_LAUNCH(k_vcluster_link, walk)
    VCL_LAUNCH(k_vcluster_roots, walk)
    VCL_LAUNCH(k_vcluster_count, waves)
    VCL_LAUNCH(k_vcluster_scan, dim3(1))
    VCL_LAUNCH(k_vcluster_rank, waves)
    VCL_LAUNCH(k_vcluster_stats, walk)
    VCL_LAUNCH(k_vcluster_resolve, walk)
#undef VCL_LAUNCH
    return hipSuccess;
}

}  // namespace sv
