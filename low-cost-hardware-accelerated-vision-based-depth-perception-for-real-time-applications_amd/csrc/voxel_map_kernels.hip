// A world-fixed voxel map: the rows of per-frame clouds (voxel rows or compact clouds), moved into the world by one pose per frame,
// accumulated per cubic cell in a table that persists from call to call, and read out as one row per voxel.  Specified in
// include/stereo_vision_hip.h (Q), restated in stereo_vision/sv.py: voxel_map_insert / voxel_map_rows.
//
//   world     Pw[k] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k] in double, every product and sum rounded on its own (no FMA: the build
//             has -ffp-contract=off); an f32 row is widened first
//   kept      weight > 0 and lo < Pw < hi on every axis (NaN and inf never pass); a row of the frame that is not kept counts into `dropped`
//   cell      (I)'s: per axis t = (Pw - lo) / size, c = min((int64)t, n - 1), u = min((int64)((t - c) * 65536), 65535); key = c_x |
//             c_y << 20 | c_z << 40 < 2^60, so the all-ones word is free to mean "empty"
//   table     open addressing with linear probing, `slots` (a power of two >= 2 * capacity) entries of eleven 64-bit words:
//             key | n | S[3] | C[4] | m | first_seq, last_seq.  An entry only ever meets integer atomics whose result does not depend on
//             their order (CAS on the key, min on first_seq, max on last_seq, add on the rest), so the table holds the same values
//             whatever the schedule was; WHERE an entry lies does depend on it, and no value does.
//   widths    the contract is a total weight below 2^47 per voxel: S_k <= 65535 n < 2^63, C_j <= 255 n < 2^55, m <= n.  A lane's
//             payload (w <= 2^31 - 1: w u < 2^47, w c < 2^39) and the sums of a wavefront's run (<= 64 lanes) travel as 64 bits.
//   insert    a lane per input row.  The claims of a wavefront (a claim is the CAS that turns an empty key into ours) count into the head
//             with one add behind the probing, not one per claim (7 % fewer atomics into an empty map; the time is the same); the
//             add that exceeds the capacity sets the sticky overflow flag, and wavefronts that see it stop.  A probe sequence is
//             bounded by `slots` - a table that fills up before the flag is seen (slots >= 2 * capacity) ends it there, and that
//             sets the flag as well -; a lane never waits for another one: a CAS that finds someone else's key moves on.  With `combine` the lanes of a wavefront
//             are split into runs of equal keys (neighbouring rows of a dense cloud mostly share a cell) and the last lane of a run
//             updates the table with the run's sums from a segmented scan; m follows from the run's length, and the sequence number is
//             the frame's, which a workgroup shares.
//   rows      tile = VMAP_TILE slots and one wavefront: the qualifying slots per tile, their exclusive prefix sum (one workgroup, the
//             scan of cloud_kernels.hip), then the rows in slot order with the rank from a ballot.  Plain loads: a kernel boundary lies
//             between the insert and the read-out.
// The world, kept and cell rules, the entry's words and the parts of the buffer are voxel_map_table.h's, which match, carry and carve
// share.
//
// Every load of the input is guarded by row < min(counts[b], cap), every slot index is masked by slots - 1, every store of a row by
// row < out_capacity; a tile index is < slots / VMAP_TILE.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_map_kernels.h"
#include "voxel_map_table.h"
#include "wave_ops.h"

namespace sv {

namespace {

__global__ __launch_bounds__(256) void k_vmap_clear(VoxelMapArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // 16-byte unit of the buffer
    if (i * 16 >= vmap_bytes(a.log2_slots)) return;
    const size_t head_words = VMAP_HEAD_BYTES / 8, table_words = (size_t)VMAP_ENTRY_WORDS << a.log2_slots;
    unsigned long long w[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const size_t word = 2 * i + k;
        w[k] = 0ull;
        if (word >= head_words && word - head_words < table_words) {
            const unsigned r = (unsigned)((word - head_words) % VMAP_ENTRY_WORDS);
            w[k] = r == VMAP_KEY ? VMAP_EMPTY : (r == VMAP_SEQ ? VMAP_SEQ_CLEARED : 0ull);
        }
    }
    *reinterpret_cast<ulonglong2 *>(a.map + i * 16) = make_ulonglong2(w[0], w[1]);
}

// Adds a run (m rows of frame `seq`, weight n, offset sums S, colour sums C) to the voxel `key`; true where that claimed a slot.
// The probe loop is vmap_claim's (voxel_map_table.h), restated around the update and the `issued` count: with the update behind the
// loop instead, as the carry has it, the kernels without `combine` take three to four more vector registers.
// tests/test_voxel_map.py holds the two texts against each other.
template <bool COUNT_ATOMICS>
__device__ __forceinline__ bool vmap_add(const VoxelMapArgs &a, uint32_t *head, unsigned long long key, unsigned long long n, unsigned long long m, uint32_t seq,
                                         const unsigned long long *S, const unsigned long long *C, bool colors) {
    unsigned long long *table = vmap_table(a.map);
    const int log2_slots = a.log2_slots;
    const uint32_t last = (uint32_t)(((size_t)1 << log2_slots) - 1);
    uint32_t h = vmap_slot_of(log2_slots, key), issued = 0;
    for (uint32_t probe = 0; probe <= last; probe++, h = (h + 1) & last) {
        if ((probe & 15) == 15 && vmap_overflowed_meanwhile(head)) break;
        unsigned long long *e = table + (size_t)h * VMAP_ENTRY_WORDS;
        const unsigned long long old = atomicCAS(e + VMAP_KEY, VMAP_EMPTY, key);
        issued++;
        if (old != VMAP_EMPTY && old != key) continue;  // someone else's: the next slot
        atomicAdd(e + VMAP_N, n);
#pragma unroll
        for (int k = 0; k < 3; k++) atomicAdd(e + VMAP_S + k, S[k]);
        if (colors) {
#pragma unroll
            for (int j = 0; j < 4; j++) atomicAdd(e + VMAP_C + j, C[j]);
        }
        atomicAdd(e + VMAP_M, m);
        uint32_t *fl = reinterpret_cast<uint32_t *>(e + VMAP_SEQ);
        atomicMin(fl, seq);
        atomicMax(fl + 1, seq);
        issued += colors ? 11 : 7;
        if (COUNT_ATOMICS) atomicAdd(a.counters, 1ull), atomicAdd(a.counters + 1, (unsigned long long)issued);
        return old == VMAP_EMPTY;
    }
    atomicOr(head + 1, 1u);  // no slot within `slots` probes: more voxels than the capacity
    if (COUNT_ATOMICS) atomicAdd(a.counters + 1, (unsigned long long)issued + 1);
    return false;
}

template <int DT, bool COMBINE, bool COUNT_ATOMICS>
__global__ __launch_bounds__(64 * VMAP_WAVES) void k_vmap_insert(VoxelMapArgs a) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const long long i = (long long)blockIdx.x * (64 * VMAP_WAVES) + threadIdx.x;  // the frame's row
    const int cnt = vmap_rows_of(a.counts, b, a.cap);
    if (i - lane >= cnt) return;  // the whole wavefront: no row of the frame in it (a count <= 0 included)
    uint32_t *head = vmap_head(a.map);
    if (__shfl(vmap_overflowed_meanwhile(head), 0)) return;  // the whole wavefront: the map's content means nothing any more
    const bool valid = i < cnt, colors = a.color != nullptr;
    const size_t o = (size_t)b * a.cap + (size_t)(valid ? i : 0);
    const double *pose = a.poses + (size_t)b * 12;
    bool keep = valid;
    double x = 0.0, y = 0.0, z = 0.0;
    long long wt = 1;
    if (valid) {
        vmap_load_row<DT>(a.xyz, o, x, y, z);
        if (a.weight) wt = a.weight[o];
        keep = wt > 0;
    }
    unsigned long long key = 0;
    uint32_t u[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double t;
        long long c;
        keep = vmap_cell(a, pose, k, x, y, z, keep, t, c);
        u[k] = (uint32_t)vmap_offset(t, c);
        key |= vmap_key_part(c, k);
    }
    if (!keep) key = VMAP_EMPTY;
    const int n_dropped = __popcll(__ballot(valid && !keep));
    if (lane == 0 && n_dropped) atomicAdd(vmap_dropped(a.map), (unsigned long long)n_dropped);

    unsigned long long n = (unsigned long long)wt, m = 1, S[3], C[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
    for (int k = 0; k < 3; k++) S[k] = n * u[k];
    if (keep && colors) {
        const uint32_t c = reinterpret_cast<const uint32_t *>(a.color)[o];
        C[0] = n * (c & 255u), C[1] = n * ((c >> 8) & 255u), C[2] = n * ((c >> 16) & 255u), C[3] = n * (c >> 24);
    }
    bool issue = keep;
    if (COMBINE) {  // every lane of the wavefront gets here
        const WaveRun run = wave_run(key);
        wave_run_scan(run, [&](int d, bool take) {  // the tail holds the run's sums
            const unsigned long long tn = __shfl_up(n, d), s0 = __shfl_up(S[0], d), s1 = __shfl_up(S[1], d), s2 = __shfl_up(S[2], d);
            unsigned long long c[4] = {0ull, 0ull, 0ull, 0ull};
            if (colors) {
#pragma unroll
                for (int j = 0; j < 4; j++) c[j] = __shfl_up(C[j], d);
            }
            if (take) {
                n += tn, S[0] += s0, S[1] += s1, S[2] += s2;
#pragma unroll
                for (int j = 0; j < 4; j++) C[j] += c[j];
            }
        });
        m = (unsigned long long)(lane - run.head_lane + 1);  // the run's lanes are all kept rows
        issue = keep && run.tail;
    }
    bool claimed = false;
    if (issue) claimed = vmap_add<COUNT_ATOMICS>(a, head, key, n, m, (uint32_t)(a.seq0 + b), S, C, colors);
    const uint32_t n_claimed = (uint32_t)__popcll(__ballot(claimed));  // every lane of the wavefront gets here
    if (lane == 0 && n_claimed) {
        const bool over = atomicAdd(head, n_claimed) + n_claimed > (uint32_t)a.capacity;
        if (over) atomicOr(head + 1, 1u);
        if (COUNT_ATOMICS) atomicAdd(a.counters + 1, over ? 2ull : 1ull);
    }
}

// Is slot h's entry a row of the read-out?
__device__ __forceinline__ bool qualifies(const VoxelMapArgs &a, const unsigned long long *e) {
    return e[VMAP_KEY] != VMAP_EMPTY && vmap_passes(a, e);
}

__global__ __launch_bounds__(64 * VMAP_WAVES) void k_vmap_count(VoxelMapArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t tile = blockIdx.x * VMAP_WAVES + (threadIdx.x >> 6);
    const uint32_t n_tiles = (uint32_t)(((size_t)1 << a.log2_slots) / VMAP_TILE);
    if (tile >= n_tiles) return;  // the whole wavefront
    const unsigned long long *table = vmap_table(a.map);
    int total = 0;
    if (!vmap_overflowed_before(a.map)) {
        for (int s = 0; s < VMAP_TILE / 64; s++) {
            const size_t h = (size_t)tile * VMAP_TILE + (size_t)(s * 64 + lane);
            total += __popcll(__ballot(qualifies(a, table + h * VMAP_ENTRY_WORDS)));
        }
    }
    if (lane == 0) vmap_tiles(a.map, a.log2_slots)[tile] = total;
}

__global__ __launch_bounds__(256) void k_vmap_scan(VoxelMapArgs a) {
    __shared__ int s_wave[4];
    const int tid = threadIdx.x;
    int32_t *tiles = vmap_tiles(a.map, a.log2_slots);
    const int n_tiles = (int)(((size_t)1 << a.log2_slots) / VMAP_TILE);  // 4 .. 2^19
    const int per = (n_tiles + 255) / 256;
    const int lo = tid * per < n_tiles ? tid * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    int own = 0;
    for (int k = lo; k < hi; k++) own += tiles[k];
    int total;
    int run = block_exclusive_scan<256>(own, s_wave, &total);  // every thread gets here
    for (int k = lo; k < hi; k++) {
        const int c = tiles[k];
        tiles[k] = run;
        run += c;
    }
    if (tid == 255) *a.count_out = vmap_overflowed_before(a.map) ? -1 : run;  // the last thread's run ends at the total (<= slots <= 2^27)
}

template <int DT>
__global__ __launch_bounds__(64 * VMAP_WAVES) void k_vmap_write(VoxelMapArgs a) {
    const int lane = threadIdx.x & 63;
    const uint32_t tile = blockIdx.x * VMAP_WAVES + (threadIdx.x >> 6);
    const uint32_t n_tiles = (uint32_t)(((size_t)1 << a.log2_slots) / VMAP_TILE);
    if (tile >= n_tiles) return;  // the whole wavefront
    if (vmap_overflowed_before(a.map)) return;  // no rows
    int row = vmap_tiles(a.map, a.log2_slots)[tile];
    for (int s = 0; s < VMAP_TILE / 64 && row < a.out_capacity; s++) {  // rows only grow: nothing later is stored either
        const size_t h = (size_t)tile * VMAP_TILE + (size_t)(s * 64 + lane);
        const unsigned long long *e = vmap_table(a.map) + h * VMAP_ENTRY_WORDS;
        const bool q = qualifies(a, e);
        const unsigned long long mask = __ballot(q);
        const int r = row + lanes_below(mask);
        row += __popcll(mask);
        if (!q || r >= a.out_capacity) continue;
        const unsigned long long key = e[VMAP_KEY], n = e[VMAP_N];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int32_t ci = vmap_key_cell(key, k);
            const double p = vmap_centre(a.lo[k], a.size, key, k, e[VMAP_S + k], n);
            if (DT == VMAP_F32) static_cast<float *>(a.xyz_out)[3 * (size_t)r + k] = (float)p;
            else static_cast<double *>(a.xyz_out)[3 * (size_t)r + k] = p;
            if (a.cell_out) a.cell_out[3 * (size_t)r + k] = ci;
        }
        if (a.color_out) {
            uint32_t c = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) c |= (uint32_t)((2ull * e[VMAP_C + j] + n) / (2ull * n)) << (8 * j);  // <= 255
            reinterpret_cast<uint32_t *>(a.color_out)[r] = c;
        }
        if (a.n_out) a.n_out[r] = (long long)n;
        if (a.m_out) a.m_out[r] = (long long)e[VMAP_M];
        if (a.first_out) a.first_out[r] = (int32_t)vmap_first_seq(e[VMAP_SEQ]);
        if (a.last_out) a.last_out[r] = (int32_t)vmap_last_seq(e[VMAP_SEQ]);
        a.key_out[r] = (long long)key;
    }
}

template <int DT>
hipError_t launch_insert_dt(bool combine, const VoxelMapArgs &a, int batch, hipStream_t st) {
    const dim3 grid((unsigned)(((long long)a.cap + 64 * VMAP_WAVES - 1) / (64 * VMAP_WAVES)), batch), block(64 * VMAP_WAVES);
    if (combine) {
        if (a.counters) hipLaunchKernelGGL((k_vmap_insert<DT, true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_vmap_insert<DT, true, false>), grid, block, 0, st, a);
    } else {
        if (a.counters) hipLaunchKernelGGL((k_vmap_insert<DT, false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_vmap_insert<DT, false, false>), grid, block, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_voxel_map_clear(const VoxelMapArgs &a, hipStream_t st) {
    const size_t units = vmap_bytes(a.log2_slots) / 16;  // < 2^30 threads: slots <= 2^27
    hipLaunchKernelGGL(k_vmap_clear, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_voxel_map_insert(int dtype, bool combine, const VoxelMapArgs &a, int batch, hipStream_t st) {
    if (dtype == VMAP_F32) return launch_insert_dt<VMAP_F32>(combine, a, batch, st);
    if (dtype == VMAP_F64) return launch_insert_dt<VMAP_F64>(combine, a, batch, st);
    return hipErrorInvalidValue;
}

hipError_t launch_voxel_map_rows(int dtype, const VoxelMapArgs &a, hipStream_t st) {
    if (dtype != VMAP_F32 && dtype != VMAP_F64) return hipErrorInvalidValue;
    const unsigned n_tiles = (unsigned)(((size_t)1 << a.log2_slots) / VMAP_TILE);
    const dim3 grid((n_tiles + VMAP_WAVES - 1) / VMAP_WAVES), block(64 * VMAP_WAVES);
    hipLaunchKernelGGL(k_vmap_count, grid, block, 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    hipLaunchKernelGGL(k_vmap_scan, dim3(1), dim3(256), 0, st, a);
    if (hipGetLastError() != hipSuccess) return hipErrorLaunchFailure;
    if (dtype == VMAP_F32) hipLaunchKernelGGL(k_vmap_write<VMAP_F32>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(k_vmap_write<VMAP_F64>, grid, block, 0, st, a);
    return hipGetLastError();
}

}  // namespace sv
