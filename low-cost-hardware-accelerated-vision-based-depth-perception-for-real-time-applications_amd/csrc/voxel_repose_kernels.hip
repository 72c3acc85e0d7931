// The voxels of one world-fixed voxel map, each moved by the rigid correction of the frame that saw it last, added into another:
// include/stereo_vision_hip.h (AD), restated in stereo_vision/sv.py (voxel_map_repose).  Both buffers are voxel_map_kernels.h's; the
// source is only read.  The filters, the centre, the transform, the way into a cell and the claiming probe are voxel_map_table.h's, the
// insert's and the read-out's own.
//
//   head    one wavefront, in front of the table kernel in stream order: the carry's head - the four counts zeroed, the source's
//           `dropped` added to the destination's, and the verdict "nothing is carried" (either map is overflowed as the call starts)
//           stored in the first word of the destination's read-out scratch, set as its overflow flag and reported as carried = -1.
//   table   a lane per source slot and trip, as the carry walks it.  A lane reads its key, for an occupied slot the three words the
//           filters need, for a voxel that qualifies (the filters, and n >= 1: the centre divides by n) the three offset sums, and the
//           five words left only for a voxel that is carried.  The centre p is vmap_centre's on three axes; the correction is
//           corr[min(max(last_seq - seq0, 0), n_corr - 1)], twelve doubles gathered through the L2 - neighbouring slots are hashed apart,
//           so neighbouring lanes read unrelated frames' rows -; vmap_cell gives the kept rule, t and the cell per axis of the
//           destination, vmap_offset the offset u, vmap_claim the entry.
//
// Many source voxels may land in one destination cell - a rigid motion is not a bijection of cells -, so an entry is changed by the
// insert's atomics and by nothing else: 64-bit integer adds on n, S[3], C[4] and m, the 32-bit minimum and maximum on the two halves of
// the sequence word.  No float atomic: every sum is an integer, so the table holds the same values whatever the schedule was.  Equal
// destination cells do not sit in neighbouring lanes of a hashed source table, so there is no merge of a wavefront's runs in front of
// the atomics.
//
// Counts and the claims leave a workgroup once, behind its last trip, as in the carry: ballots into registers, the four wavefronts'
// counts added in LDS, one add per counter; the add of claims that exceeds the capacity sets the sticky overflow flag.  The probe is
// bounded by `slots` and looks at the flag every sixteenth step (vmap_claim), so every loop ends by the data alone.
//
// Every load of the source is at slot < slots of the source (the loop's bound), every load of corr at a row in 0 .. n_corr - 1 (the
// clamp), every slot index of the destination is masked by its slots - 1.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_table.h"
#include "voxel_repose_kernels.h"

namespace sv {

namespace {

__global__ __launch_bounds__(64) void k_vrepose_head(VoxelReposeArgs a) {
    if (threadIdx.x != 0) return;
    const bool lost = vmap_overflowed_before(a.src) || vmap_overflowed_before(a.dst);
    vmap_tiles(a.dst, a.dst_log2_slots)[0] = lost ? 1 : 0;
    *vmap_dropped(a.dst) += *vmap_dropped(a.src);
    if (lost) vmap_head(a.dst)[1] = 1u;
    if (a.stats) {
        a.stats[0] = lost ? -1ll : 0ll;
        for (int k = 1; k < VREPOSE_STATS; k++) a.stats[k] = 0ll;
    }
}

// One row of weight n at offsets u, with the source entry's colour sums, rows and sequences, added to the voxel `key` of the
// destination; true where that claimed a slot.  Other lanes may add to the same entry meanwhile: atomics only.
__device__ __forceinline__ bool repose_entry(const VoxelReposeArgs &a, unsigned long long key, const unsigned long long *e, unsigned long long n, const long long *u,
                                             unsigned long long m, unsigned long long seqs) {
    bool claimed;
    unsigned long long *d = vmap_claim(vmap_head(a.dst), vmap_table(a.dst), a.dst_log2_slots, key, claimed);
    if (!d) return false;
    atomicAdd(d + VMAP_N, n);
#pragma unroll
    for (int k = 0; k < 3; k++) atomicAdd(d + VMAP_S + k, n * (unsigned long long)u[k]);  // n < 2^47, u < 2^16
#pragma unroll
    for (int j = 0; j < 4; j++) atomicAdd(d + VMAP_C + j, e[VMAP_C + j]);
    atomicAdd(d + VMAP_M, m);
    uint32_t *fl = reinterpret_cast<uint32_t *>(d + VMAP_SEQ);
    atomicMin(fl, vmap_first_seq(seqs));
    atomicMax(fl + 1, vmap_last_seq(seqs));
    return claimed;
}

__global__ __launch_bounds__(VREPOSE_THREADS) void k_vrepose_table(VoxelReposeArgs a) {
    __shared__ uint32_t s_count[VREPOSE_THREADS / 64][VREPOSE_STATS];
    if (vmap_tiles(a.dst, a.dst_log2_slots)[0]) return;  // the whole grid: a map was overflowed as the call started
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t slots = (size_t)1 << a.src_log2_slots;  // a multiple of VREPOSE_THREADS
    uint32_t n_carried = 0, n_filtered = 0, n_outside = 0, n_claimed = 0;  // of this wavefront, over its trips: at most slots <= 2^27
    for (size_t slot = (size_t)blockIdx.x * VREPOSE_THREADS + threadIdx.x; slot < slots; slot += (size_t)gridDim.x * VREPOSE_THREADS) {  // the same trips for a workgroup
        const unsigned long long *e = vmap_table(a.src) + slot * VMAP_ENTRY_WORDS;
        const unsigned long long key = e[VMAP_KEY];
        const bool occupied = key != VMAP_EMPTY;
        unsigned long long n = 0, m = 0, seqs = 0;
        bool q = false;
        if (occupied) {
            n = e[VMAP_N], m = e[VMAP_M], seqs = e[VMAP_SEQ];
            q = vmap_passes(a, e) && (long long)n >= 1;  // a tombstone never qualifies: the centre divides by n
        }
        bool inside = q;
        unsigned long long moved = 0;
        long long u[3] = {0, 0, 0};
        if (q) {
            const double x = vmap_centre(a.src_lo[0], a.src_size, key, 0, e[VMAP_S], n);
            const double y = vmap_centre(a.src_lo[1], a.src_size, key, 1, e[VMAP_S + 1], n);
            const double z = vmap_centre(a.src_lo[2], a.src_size, key, 2, e[VMAP_S + 2], n);
            long long at = (long long)(int32_t)vmap_last_seq(seqs) - (long long)a.seq0;
            at = at < 0 ? 0 : at > (long long)a.n_corr - 1 ? (long long)a.n_corr - 1 : at;
            const double *pose = a.corr + 12 * (size_t)at;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                double t;
                long long c;
                inside = vmap_cell(a, pose, k, x, y, z, inside, t, c);
                u[k] = vmap_offset(t, c);  // used where inside
                moved |= vmap_key_part(c, k);
            }
        }
        bool claimed = false;
        if (inside) claimed = repose_entry(a, moved, e, n, u, m, seqs);
        // every lane of the wavefront gets here
        n_claimed += (uint32_t)__popcll(__ballot(claimed)), n_carried += (uint32_t)__popcll(__ballot(inside));
        n_filtered += (uint32_t)__popcll(__ballot(occupied && !q)), n_outside += (uint32_t)__popcll(__ballot(q && !inside));
    }
    // The counts of the workgroup leave it once, behind its last trip, as the carry's do.
    if (lane == 0) s_count[wave][0] = n_carried, s_count[wave][1] = n_filtered, s_count[wave][2] = n_outside, s_count[wave][3] = n_claimed;
    __syncthreads();  // every thread of the workgroup gets here
    if (threadIdx.x >= VREPOSE_STATS) return;
    uint32_t total = 0;
    for (int w = 0; w < VREPOSE_THREADS / 64; w++) total += s_count[w][threadIdx.x];
    if (total == 0) return;
    if (threadIdx.x == VREPOSE_STATS - 1) {  // the claims: the insert's rule
        uint32_t *head = vmap_head(a.dst);
        const bool over = atomicAdd(head, total) + total > (uint32_t)a.dst_capacity;
        if (over) atomicOr(head + 1, 1u);
    }
    if (a.stats) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + threadIdx.x, (unsigned long long)total);
}

}  // namespace

hipError_t launch_voxel_repose(const VoxelReposeArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_vrepose_head, dim3(1), dim3(64), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    const size_t tiles = ((size_t)1 << a.src_log2_slots) / VREPOSE_THREADS;  // slots is a multiple of VREPOSE_THREADS: >= 1024
    hipLaunchKernelGGL(k_vrepose_table, dim3((unsigned)(tiles < VREPOSE_MAX_GROUPS ? tiles : VREPOSE_MAX_GROUPS)), dim3(VREPOSE_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
