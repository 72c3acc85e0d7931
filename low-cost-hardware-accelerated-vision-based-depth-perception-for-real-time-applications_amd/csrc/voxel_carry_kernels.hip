// The voxels of one world-fixed voxel map, filtered and shifted by whole cells, added into another: include/stereo_vision_hip.h (S),
// restated in stereo_vision/sv.py (voxel_map_carry).  Both buffers are voxel_map_kernels.h's; the source is only read.  slot_of and the
// read-out's three filters are voxel_map_kernels.hip's, restated here (tests/test_voxel_carry.py holds the texts against each other).
//
//   head    one wavefront, in front of the table kernel in stream order: the four counts zeroed, the source's `dropped` added to the
//           destination's, and the verdict "nothing is carried" - either map is overflowed as the call starts - stored in the first word
//           of the destination's read-out scratch, set as the destination's overflow flag and reported as carried = -1.
//   table   a lane per source slot and trip; a wavefront's 64 entries are 5632 contiguous bytes.  A lane reads its key, for an occupied
//           slot the three words the filters need, and the other seven only for a voxel that is carried.  The destination entry of a
//           carried voxel is found as the insert finds it - linear probing from slot_of, bounded by `slots`, indices masked by slots -
//           1, a CAS on the key that moves on at someone else's key - and then changed with plain loads, adds, min / max and stores.
//
// Precondition of the plain stores: within a call a destination entry is touched by exactly one lane.  The keys of the source are
// distinct, the shift maps distinct keys to distinct keys, so no two lanes carry the same key and each settles on an entry of its own;
// another lane only ever meets that entry's key word, with its CAS.  No other call on either map runs meanwhile (the C entry's contract),
// and what the destination held before was written in front of a kernel boundary.  A cleared entry - first_seq all ones, zeros
// elsewhere - is the neutral element of every update, so a claimed entry and a found one are the same code.
//
// A workgroup walks the source in strides of the grid (at most VCARRY_MAX_GROUPS workgroups).  Its wavefronts count by ballots into
// registers; behind the last trip the four wavefronts' counts are added in LDS and leave the workgroup as one add per counter.  The
// claims count into the head the same way, and the add that exceeds the capacity sets the sticky overflow flag: the insert's rule, at
// a workgroup's grain.  A lane looks at the flag every sixteenth probe and gives up where it is set, and a probe sequence that ends
// without a slot sets it, so a destination that is too small ends the call early whatever the counts say.
//
// Every load of the source is at slot < slots of the source (the loop's bound), every slot index of the destination is masked by its
// slots - 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_carry_kernels.h"

namespace sv {

namespace {

constexpr unsigned long long VMAP_EMPTY = ~0ull;

// The destination, as the probing needs it.
struct CarryTable {
    uint32_t *head;  // [0] claimed slots, [1] overflowed
    unsigned long long *table;
    int log2_slots, capacity;
};

__device__ __forceinline__ uint32_t slot_of(const CarryTable &a, unsigned long long key) {
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> (64 - a.log2_slots));  // log2_slots in 10 .. 27
}

__device__ __forceinline__ uint32_t overflowed(const uint32_t *head) { return __hip_atomic_load(head + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int32_t *tiles_of(uint8_t *map, int log2_slots) {
    return reinterpret_cast<int32_t *>(map + VMAP_HEAD_BYTES + ((size_t)VMAP_ENTRY_WORDS * 8 << log2_slots));
}

__global__ __launch_bounds__(64) void k_vcarry_head(VoxelCarryArgs a) {
    if (threadIdx.x != 0) return;
    uint32_t *dh = reinterpret_cast<uint32_t *>(a.dst);
    const uint32_t *sh = reinterpret_cast<const uint32_t *>(a.src);
    const bool lost = sh[1] != 0u || dh[1] != 0u;
    tiles_of(a.dst, a.dst_log2_slots)[0] = lost ? 1 : 0;
    *reinterpret_cast<unsigned long long *>(a.dst + 8) += *reinterpret_cast<const unsigned long long *>(a.src + 8);  // dropped
    if (lost) dh[1] = 1u;
    if (a.stats) {
        a.stats[0] = lost ? -1ll : 0ll;
        for (int k = 1; k < VCARRY_STATS; k++) a.stats[k] = 0ll;
    }
}

// Adds the source entry e to the voxel `key` of the destination; true where that claimed a slot.  See the precondition above.
__device__ __forceinline__ bool carry_entry(const CarryTable &a, unsigned long long key, const unsigned long long *e, unsigned long long n, unsigned long long m,
                                            unsigned long long seqs) {
    const uint32_t last = (uint32_t)(((size_t)1 << a.log2_slots) - 1);
    uint32_t h = slot_of(a, key);
    for (uint32_t probe = 0; probe <= last; probe++, h = (h + 1) & last) {
        if ((probe & 15) == 15 && overflowed(a.head)) break;  // a full table of a map that is lost anyway
        unsigned long long *d = a.table + (size_t)h * VMAP_ENTRY_WORDS;
        const unsigned long long old = atomicCAS(d, VMAP_EMPTY, key);
        if (old != VMAP_EMPTY && old != key) continue;  // someone else's: the next slot
        d[1] += n;
#pragma unroll
        for (int k = 2; k < 9; k++) d[k] += e[k];  // S[3], C[4]
        d[9] += m;
        const unsigned long long have = d[10];
        const uint32_t f0 = (uint32_t)have, f1 = (uint32_t)seqs, l0 = (uint32_t)(have >> 32), l1 = (uint32_t)(seqs >> 32);
        d[10] = (unsigned long long)(f0 < f1 ? f0 : f1) | (unsigned long long)(l0 > l1 ? l0 : l1) << 32;
        return old == VMAP_EMPTY;
    }
    atomicOr(a.head + 1, 1u);  // no slot within `slots` probes: more voxels than the capacity
    return false;
}

__global__ __launch_bounds__(VCARRY_THREADS) void k_vcarry_table(VoxelCarryArgs a) {
    __shared__ uint32_t s_count[VCARRY_THREADS / 64][VCARRY_STATS];
    if (tiles_of(a.dst, a.dst_log2_slots)[0]) return;  // the whole grid: a map was overflowed as the call started
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t slots = (size_t)1 << a.src_log2_slots;  // a multiple of VCARRY_THREADS
    CarryTable t;
    t.head = reinterpret_cast<uint32_t *>(a.dst);
    t.table = reinterpret_cast<unsigned long long *>(a.dst + VMAP_HEAD_BYTES);
    t.log2_slots = a.dst_log2_slots, t.capacity = a.dst_capacity;
    uint32_t n_carried = 0, n_filtered = 0, n_outside = 0, n_claimed = 0;  // of this wavefront, over its trips: at most slots <= 2^27
    for (size_t slot = (size_t)blockIdx.x * VCARRY_THREADS + threadIdx.x; slot < slots; slot += (size_t)gridDim.x * VCARRY_THREADS) {  // the same trips for a workgroup
        const unsigned long long *e = reinterpret_cast<const unsigned long long *>(a.src + VMAP_HEAD_BYTES) + slot * VMAP_ENTRY_WORDS;
        const unsigned long long key = e[0];
        const bool occupied = key != VMAP_EMPTY;
        unsigned long long n = 0, m = 0, seqs = 0;
        bool q = false;
        if (occupied) {
            n = e[1], m = e[9], seqs = e[10];
            q = (long long)n >= a.min_n && (long long)m >= a.min_rows && (int32_t)(seqs >> 32) >= a.since;  // the read-out's filters
        }
        bool inside = q;
        unsigned long long moved = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int c = (int)((key >> (20 * k)) & 0xFFFFFull) + a.shift[k];  // -2^20 .. 2^21
            inside = inside && c >= 0 && c < a.dst_nc[k];
            moved |= (unsigned long long)(uint32_t)(c & 0xFFFFF) << (20 * k);  // used where inside: c itself
        }
        bool claimed = false;
        if (inside) claimed = carry_entry(t, moved, e, n, m, seqs);
        // every lane of the wavefront gets here
        n_claimed += (uint32_t)__popcll(__ballot(claimed)), n_carried += (uint32_t)__popcll(__ballot(inside));
        n_filtered += (uint32_t)__popcll(__ballot(occupied && !q)), n_outside += (uint32_t)__popcll(__ballot(q && !inside));
    }
    // The counts of the workgroup leave it once, behind its last trip: a counter that every wavefront of every trip added to would be
    // one address under some 2^19 atomics, which is what the call would then wait for.
    if (lane == 0) s_count[wave][0] = n_carried, s_count[wave][1] = n_filtered, s_count[wave][2] = n_outside, s_count[wave][3] = n_claimed;
    __syncthreads();  // every thread of the workgroup gets here
    if (threadIdx.x >= VCARRY_STATS) return;
    uint32_t total = 0;
    for (int w = 0; w < VCARRY_THREADS / 64; w++) total += s_count[w][threadIdx.x];
    if (total == 0) return;
    if (threadIdx.x == VCARRY_STATS - 1) {  // the claims: the insert's rule
        const bool over = atomicAdd(t.head, total) + total > (uint32_t)t.capacity;
        if (over) atomicOr(t.head + 1, 1u);
    }
    if (a.stats) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + threadIdx.x, (unsigned long long)total);
}

}  // namespace

hipError_t launch_voxel_carry(const VoxelCarryArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_vcarry_head, dim3(1), dim3(64), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    const size_t tiles = ((size_t)1 << a.src_log2_slots) / VCARRY_THREADS;  // slots is a multiple of VCARRY_THREADS: >= 1024
    hipLaunchKernelGGL(k_vcarry_table, dim3((unsigned)(tiles < VCARRY_MAX_GROUPS ? tiles : VCARRY_MAX_GROUPS)), dim3(VCARRY_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
