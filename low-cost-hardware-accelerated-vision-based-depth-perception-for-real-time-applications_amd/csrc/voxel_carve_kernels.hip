// A world-fixed voxel map carved by the sight lines of frames: include/stereo_vision_hip.h (T), restated in stereo_vision/sv.py
// (voxel_map_carve).  The map's buffer is voxel_map_kernels.h's; the transform, the kept rule, the cell rule, slot_of and the read-only
// probe are voxel_map_table.h's.  Three kernels in stream order; no workgroup waits for another:
//
//   zero    miss (a 64-bit word per slot, outside the map) and stats cleared, 16 bytes per store; for an overflowed map the verdict
//           rays = -1 instead.  The "do nothing" word the other two kernels read is the map's own overflow flag: no kernel of this call
//           changes it and no other call on the map runs meanwhile, so it needs no copy - and a call with apply = 0 stores nothing into
//           the map at all.
//   rays    grid (ceil(cap / 256), frame), a lane per row.  Thread 0 works out whether the frame casts and the sensor's cell c0 - twelve
//           pose words that must be finite, the insert's transform of `origin`, lo < O < hi, the insert's cell rule - and leaves them in
//           LDS: once per workgroup.  A lane does the insert's transform and cell rule for its row, then walks k = 1 .. nst - 1 - margin
//           with three error accumulators (occupancy_map_cells.h: line_step, the flat map's): per axis c0 + (2 k d + nst) // (2 nst) with
//           a flooring division, term by term (|2 k d + nst| < 2^22 at reach <= 1023).  VCARVE_STEPS steps make a trip: their keys, then
//           the first probe of each - independent loads, in flight together -, then for a first slot that holds another key the whole
//           read-only linear probe from slot_of (ended by the key, by an empty key or after `slots` probes), then the found entries'
//           last words.  Where last_seq lies before the frame's number the row's weight is added to miss[slot] with a 64-bit integer
//           atomic - the stage's only one, order-free.  In front of it the lanes of the wavefront are split into runs of equal slots
//           (wave_run) and a run's last lane adds the run's sum: neighbouring rows are neighbouring cells, and near the sensor, where
//           every ray of the frame passes through the same few voxels, their rays share cells.  For that every lane of a wavefront
//           walks as far as the wavefront's longest ray; a lane beyond its own last step looks nothing up and adds nothing.  rays and
//           steps are per-lane counters, summed per wavefront (wave_ops.h), then per workgroup in LDS: one add per counter and
//           workgroup.
//   apply   a lane per slot and trip, walking in strides of the grid.  miss[slot] first; the entry's n only where miss > 0; the ten
//           value words go back to a cleared entry's - first_seq all ones, zeros elsewhere - with plain stores, for a carved voxel under
//           `apply` only.  The key stays: a tombstone, so probe chains through it hold.  The entry belongs to that lane alone.  touched
//           and carved count by ballots into registers and leave the workgroup as one add per counter.
//
// Bounds: every load of a row is guarded by row < min(counts[b], cap); every slot index is masked by slots - 1; a step's cell lies
// between c0 and c1 on every axis, both of which the cell rule clamps into the box, so every key is one of a cell of the box; a step
// beyond a ray's last is given the empty key and loads nothing; the step loop of a wavefront ends after its longest ray, at most reach - 1
// steps, and a probe after `slots`; miss has `slots` words (the C entry's contract).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occupancy_map_cells.h"
#include "voxel_carve_kernels.h"
#include "voxel_map_table.h"
#include "wave_ops.h"

namespace sv {

namespace {

__global__ __launch_bounds__(VCARVE_THREADS) void k_vcarve_zero(VoxelCarveArgs a) {
    const size_t slots = (size_t)1 << a.log2_slots;
    // 16-byte units from the 16-byte boundary at or below miss: unit u holds the words 2 u - off and 2 u - off + 1
    const size_t off = (reinterpret_cast<uintptr_t>(a.miss) >> 3) & 1, units = (slots + off + 1) / 2;
    const size_t u = (size_t)blockIdx.x * VCARVE_THREADS + threadIdx.x;
    if (u < units) {
        const long long w0 = 2 * (long long)u - (long long)off;
        if (w0 >= 0 && (size_t)w0 + 1 < slots) *reinterpret_cast<ulonglong2 *>(a.miss + w0) = make_ulonglong2(0ull, 0ull);
        else a.miss[w0 >= 0 ? w0 : 0] = 0ull;  // the first word of a buffer that starts on an odd word, or its last
    }
    if (u == 0 && a.stats) {
        a.stats[0] = vmap_overflowed_before(a.map) ? -1ll : 0ll;
        for (int k = 1; k < VCARVE_STATS; k++) a.stats[k] = 0ll;
    }
}

template <int DT>
__global__ __launch_bounds__(VCARVE_THREADS) void k_vcarve_rays(VoxelCarveArgs a) {
    __shared__ int s_c0[4];  // the sensor's cell, and whether the frame casts
    __shared__ unsigned long long s_count[VCARVE_THREADS / 64][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
    const long long i = (long long)blockIdx.x * VCARVE_THREADS + threadIdx.x;  // the frame's row
    const int cnt = vmap_rows_of(a.counts, b, a.cap);
    if ((long long)blockIdx.x * VCARVE_THREADS >= cnt) return;  // the whole workgroup: no row of the frame in it (a count <= 0 included)
    if (vmap_overflowed_before(a.map)) return;  // the whole grid
    const double *pose = a.poses + (size_t)b * 12;
    if (threadIdx.x == 0) {
        bool keep = true;
        for (int k = 0; k < 12; k++) keep = keep && __builtin_isfinite(pose[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            double t;
            long long c;
            keep = vmap_cell(a, pose, k, a.origin[0], a.origin[1], a.origin[2], keep, t, c);
            s_c0[k] = (int)c;
        }
        s_c0[3] = keep ? 1 : 0;
    }
    __syncthreads();  // every thread of the workgroup gets here
    const bool casts = s_c0[3] != 0;

    const bool valid = i < cnt;
    const size_t o = (size_t)b * a.cap + (size_t)(valid ? i : 0);
    bool keep = valid && casts;
    double x = 0.0, y = 0.0, z = 0.0;
    long long wt = 1;
    if (keep) {
        vmap_load_row<DT>(a.xyz, o, x, y, z);
        if (a.weight) wt = a.weight[o];
        keep = wt > 0;
    }
    int d[3], nst = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double t;
        long long c;
        keep = vmap_cell(a, pose, k, x, y, z, keep, t, c);
        d[k] = (int)c - s_c0[k];  // |d| < 2^20
        const int m = d[k] < 0 ? -d[k] : d[k];
        nst = m > nst ? m : nst;
    }
    const bool ray = keep && nst <= a.reach;
    const int n_steps = ray && nst - 1 - a.margin > 0 ? nst - 1 - a.margin : 0;  // <= reach - 1

    const unsigned long long *table = vmap_table(a.map);
    const uint32_t seq = (uint32_t)(a.seq0 + b);
    int c[3] = {s_c0[0], s_c0[1], s_c0[2]}, rem[3] = {nst, nst, nst};  // 2 k d + nst = (c - c0) * 2 nst + rem, 0 <= rem < 2 nst
    const int n_most = wave_max(n_steps);  // every lane of the wavefront gets here, and walks as far as its longest ray: the merge below shuffles
    for (int k0 = 1; k0 <= n_most; k0 += VCARVE_STEPS) {  // VCARVE_STEPS steps at a time: their loads are in flight together
        unsigned long long key[VCARVE_STEPS], word[VCARVE_STEPS];
        uint32_t h[VCARVE_STEPS];
#pragma unroll
        for (int u = 0; u < VCARVE_STEPS; u++) {
#pragma unroll
            for (int j = 0; j < 3; j++) line_step(rem[j], c[j], 2 * d[j], 2 * nst);  // |2 d| <= 2 nst: one wrap at most
            // a step beyond the ray's last is not looked up: its cell may lie outside the box
            key[u] = k0 + u <= n_steps ? vmap_key(c[0], c[1], c[2]) : VMAP_EMPTY;
            h[u] = vmap_slot_of(a.log2_slots, key[u]);
        }
#pragma unroll
        for (int u = 0; u < VCARVE_STEPS; u++) word[u] = key[u] != VMAP_EMPTY ? table[(size_t)h[u] * VMAP_ENTRY_WORDS + VMAP_KEY] : VMAP_EMPTY;  // the first probe of each
        long long at[VCARVE_STEPS];
#pragma unroll
        for (int u = 0; u < VCARVE_STEPS; u++)  // an empty first slot: no voxel; another key there: the whole probe, which is rare
            at[u] = word[u] == VMAP_EMPTY ? -1 : (word[u] == key[u] ? (long long)h[u] : vmap_find(table, a.log2_slots, key[u]));
#pragma unroll
        for (int u = 0; u < VCARVE_STEPS; u++) word[u] = at[u] >= 0 ? table[(size_t)at[u] * VMAP_ENTRY_WORDS + VMAP_SEQ] : ~0ull;  // last_seq all ones: never older
#pragma unroll
        for (int u = 0; u < VCARVE_STEPS; u++) {
            const bool add = vmap_last_seq(word[u]) < seq;  // the voxel is older than the frame
            // neighbouring rows are neighbouring cells, and near the sensor their rays share cells: one add per run of equal slots
            const WaveRun run = wave_run(add ? at[u] : -1ll - lane);
            unsigned long long w = add ? (unsigned long long)wt : 0ull;
            wave_run_scan(run, [&](int dd, bool take) {
                const unsigned long long t = __shfl_up(w, dd);
                if (take) w += t;
            });
            if (add && run.tail) atomicAdd(a.miss + at[u], w);
        }
    }

    // every lane of the workgroup gets here
    const unsigned long long n_rays = wave_sum((unsigned long long)(ray ? 1 : 0)), n_all = wave_sum((unsigned long long)n_steps);
    if (lane == 0) s_count[wave][0] = n_rays, s_count[wave][1] = n_all;
    __syncthreads();
    if (threadIdx.x >= 2 || !a.stats) return;
    unsigned long long total = 0;
    for (int w = 0; w < VCARVE_THREADS / 64; w++) total += s_count[w][threadIdx.x];
    if (total) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + threadIdx.x, total);
}

__global__ __launch_bounds__(VCARVE_THREADS) void k_vcarve_apply(VoxelCarveArgs a) {
    __shared__ uint32_t s_count[VCARVE_THREADS / 64][2];
    if (vmap_overflowed_before(a.map)) return;  // the whole grid
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t slots = (size_t)1 << a.log2_slots;  // a multiple of VCARVE_THREADS
    uint32_t n_touched = 0, n_carved = 0;            // of this wavefront, over its trips: at most slots <= 2^27
    for (size_t slot = (size_t)blockIdx.x * VCARVE_THREADS + threadIdx.x; slot < slots; slot += (size_t)gridDim.x * VCARVE_THREADS) {  // the same trips for a workgroup
        const unsigned long long miss = a.miss[slot];
        bool carved = false;
        if (miss > 0ull) {
            unsigned long long *e = vmap_table(a.map) + slot * VMAP_ENTRY_WORDS;
            const unsigned long long n = e[VMAP_N];
            carved = (long long)miss >= a.min_miss && 256ull * miss >= (unsigned long long)a.ratio * n;  // miss, n < 2^47: both below 2^63
            if (carved && a.apply) vmap_clear_values(e);
        }
        // every lane of the wavefront gets here
        n_touched += (uint32_t)__popcll(__ballot(miss > 0ull)), n_carved += (uint32_t)__popcll(__ballot(carved));
    }
    if (lane == 0) s_count[wave][0] = n_touched, s_count[wave][1] = n_carved;
    __syncthreads();  // every thread of the workgroup gets here
    if (threadIdx.x >= 2 || !a.stats) return;
    uint32_t total = 0;
    for (int w = 0; w < VCARVE_THREADS / 64; w++) total += s_count[w][threadIdx.x];
    if (total) atomicAdd(reinterpret_cast<unsigned long long *>(a.stats) + 2 + threadIdx.x, (unsigned long long)total);
}

}  // namespace

hipError_t launch_voxel_carve(int dtype, const VoxelCarveArgs &a, int batch, hipStream_t st) {
    if (dtype != VMAP_F32 && dtype != VMAP_F64) return hipErrorInvalidValue;
    const size_t slots = (size_t)1 << a.log2_slots, units = slots / 2 + 1;  // slots is a multiple of 1024
    hipLaunchKernelGGL(k_vcarve_zero, dim3((unsigned)((units + VCARVE_THREADS - 1) / VCARVE_THREADS)), dim3(VCARVE_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (batch > 0 && a.cap > 0) {
        const dim3 grid((unsigned)(((long long)a.cap + VCARVE_THREADS - 1) / VCARVE_THREADS), (unsigned)batch);
        if (dtype == VMAP_F32) hipLaunchKernelGGL(k_vcarve_rays<VMAP_F32>, grid, dim3(VCARVE_THREADS), 0, st, a);
        else hipLaunchKernelGGL(k_vcarve_rays<VMAP_F64>, grid, dim3(VCARVE_THREADS), 0, st, a);
        if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    }
    const size_t tiles = slots / VCARVE_THREADS;
    hipLaunchKernelGGL(k_vcarve_apply, dim3((unsigned)(tiles < VCARVE_MAX_GROUPS ? tiles : VCARVE_MAX_GROUPS)), dim3(VCARVE_THREADS), 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
