// The voxels of one world-fixed voxel map, filtered and shifted by whole cells, added into another: include/stereo_vision_hip.h (S),
// restated in stereo_vision/sv.py (voxel_map_carry).  Both buffers are voxel_map_kernels.h's; the source is only read.  The read-out's
// three filters and the claiming probe are voxel_map_table.h's, the insert's own.
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
#include "voxel_map_table.h"

namespace sv {

namespace {

__global__ __launch_bounds__(64) void k_vcarry_head(VoxelCarryArgs a) {
    if (threadIdx.x != 0) return;
    const bool lost = vmap_overflowed_before(a.src) || vmap_overflowed_before(a.dst);
    vmap_tiles(a.dst, a.dst_log2_slots)[0] = lost ? 1 : 0;
    *vmap_dropped(a.dst) += *vmap_dropped(a.src);
    if (lost) vmap_head(a.dst)[1] = 1u;
    if (a.stats) {
        a.stats[0] = lost ? -1ll : 0ll;
        for (int k = 1; k < VCARRY_STATS; k++) a.stats[k] = 0ll;
    }
}

// Adds the source entry e to the voxel `key` of the destination; true where that claimed a slot.  See the precondition above.
__device__ __forceinline__ bool carry_entry(const VoxelCarryArgs &a, unsigned long long key, const unsigned long long *e, unsigned long long n, unsigned long long m,
                                            unsigned long long seqs) {
    bool claimed;
    unsigned long long *d = vmap_claim(vmap_head(a.dst), vmap_table(a.dst), a.dst_log2_slots, key, claimed);
    if (!d) return false;
    d[VMAP_N] += n;
#pragma unroll
    for (int k = VMAP_S; k < VMAP_M; k++) d[k] += e[k];  // S[3], C[4]
    d[VMAP_M] += m;
    const unsigned long long have = d[VMAP_SEQ];
    const uint32_t f0 = vmap_first_seq(have), f1 = vmap_first_seq(seqs), l0 = vmap_last_seq(have), l1 = vmap_last_seq(seqs);
    d[VMAP_SEQ] = (unsigned long long)(f0 < f1 ? f0 : f1) | (unsigned long long)(l0 > l1 ? l0 : l1) << 32;
    return claimed;
}

__global__ __launch_bounds__(VCARRY_THREADS) void k_vcarry_table(VoxelCarryArgs a) {
    __shared__ uint32_t s_count[VCARRY_THREADS / 64][VCARRY_STATS];
    if (vmap_tiles(a.dst, a.dst_log2_slots)[0]) return;  // the whole grid: a map was overflowed as the call started
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t slots = (size_t)1 << a.src_log2_slots;  // a multiple of VCARRY_THREADS
    uint32_t n_carried = 0, n_filtered = 0, n_outside = 0, n_claimed = 0;  // of this wavefront, over its trips: at most slots <= 2^27
    for (size_t slot = (size_t)blockIdx.x * VCARRY_THREADS + threadIdx.x; slot < slots; slot += (size_t)gridDim.x * VCARRY_THREADS) {  // the same trips for a workgroup
        const unsigned long long *e = vmap_table(a.src) + slot * VMAP_ENTRY_WORDS;
        const unsigned long long key = e[VMAP_KEY];
        const bool occupied = key != VMAP_EMPTY;
        unsigned long long n = 0, m = 0, seqs = 0;
        bool q = false;
        if (occupied) {
            n = e[VMAP_N], m = e[VMAP_M], seqs = e[VMAP_SEQ];
            q = vmap_passes(a, e);
        }
        bool inside = q;
        unsigned long long moved = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int c = vmap_key_cell(key, k) + a.shift[k];  // -2^20 .. 2^21
            inside = inside && c >= 0 && c < a.dst_nc[k];
            moved |= (unsigned long long)(uint32_t)(c & 0xFFFFF) << (20 * k);  // used where inside: c itself
        }
        bool claimed = false;
        if (inside) claimed = carry_entry(a, moved, e, n, m, seqs);
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
        uint32_t *head = vmap_head(a.dst);
        const bool over = atomicAdd(head, total) + total > (uint32_t)a.dst_capacity;
        if (over) atomicOr(head + 1, 1u);
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
